"""GPU: the farthest-point-sampling kernels the FPS_* options route to (csrc/geometry.hip; the ledger of
tests/options_ref.py says which test covers which option), index for index against oracle.geometry.farthest_point_sample.

FPS has no tolerance: every route must return the oracle's indices.  Each case runs B = 2 clouds with different starts on
four inputs -- uniform points with a planted duplicate (a tie at zero distance), a KITTI-shaped scan, a cloud whose points
are all the same point and a cloud on one axis (both without extent on some axis: the bounding boxes the pruned kernels
skip by degenerate to points and segments) -- twice: through pointnet_util.farthest_point_sample, which must size the
workspace AFTER the option was set, and through the C ABI (pn2_fps_workspace_bytes + pn2_fps) with the workspace and the
output in front of guard words, the workspace filled with NaN bit patterns.

pn2_fps does not record pn2_last_kernel(): that an option takes the route a test is named after rests on the dispatch code
(pn2_fps, launch_fps_pruned, fps_coop_plan), quoted in each docstring, not on an assertion.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import geometry as G
from pointnet12_amd import _lib
from pointnet12_amd import pointnet_util as U
from pointnet12_amd import synthetic as syn

import options_ref as O
from options_ref import options

pytestmark = pytest.mark.gpu

B = 2
KINDS = ("uniform", "kitti", "same", "axis")
SENTINEL = 0x7FA5A5A5
GUARD = 64                                                   # words behind the workspace / the output


@functools.lru_cache(maxsize=None)
def _cloud(kind, N):
    rng = np.random.default_rng(1000 + N + len(kind))
    if kind == "uniform":
        xyz = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        xyz[:, N // 2] = xyz[:, 0]                           # a duplicate: a tie at zero distance
    elif kind == "kitti":
        pts, _ = syn.kitti_batch(700 + N % 61, B, N)
        xyz = np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1)).astype(np.float32)
    elif kind == "same":
        xyz = np.tile(rng.uniform(-1, 1, (B, 1, 3)).astype(np.float32), (1, N, 1))
    else:
        xyz = np.zeros((B, N, 3), np.float32)
        xyz[:, :, 0] = rng.uniform(-40, 40, (B, N))
        xyz[:, N // 2] = xyz[:, 0]
    start = np.array([N // 3, N - 1], np.int64)
    return xyz, start


@functools.lru_cache(maxsize=None)
def _ref(kind, N, S):
    xyz, start = _cloud(kind, N)
    ref = G.farthest_point_sample(xyz, S, start)
    ref.setflags(write=False)
    return ref


def _abi(dev, x, st, S, ws_bytes=None, twice=False):
    """pn2_fps through the C ABI with the queried workspace (NaN patterns) and the output in front of guard words; `twice`:
    the same call again on the workspace the first one left behind."""
    lib = _lib.load()
    N = x.shape[1]
    nbytes = int(lib.pn2_fps_workspace_bytes(B, N, S))
    if ws_bytes is not None:
        assert nbytes == ws_bytes, (nbytes, ws_bytes)
    assert nbytes % 4 == 0
    work = torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2 if twice else 1):
        out = torch.full((B * S + GUARD,), -7, dtype=torch.int64, device=dev)
        rc = lib.pn2_fps(x.data_ptr(), B, N, st.data_ptr(), S, out.data_ptr(), work.data_ptr() if nbytes else None, _lib.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool((work[nbytes // 4:] == SENTINEL).all()), "written behind the workspace"
        assert bool((out[B * S:] == -7).all()), "written behind the output"
        outs.append(out[:B * S].view(B, S).cpu().numpy())
    return outs


def _check(dev, N, samples, ws_bytes=None, twice=False, kinds=KINDS):
    for S in samples:
        for kind in kinds:
            xyz, start = _cloud(kind, N)
            ref = _ref(kind, N, S)
            x, st = torch.tensor(xyz, device=dev), torch.tensor(start, device=dev)
            mine = U.farthest_point_sample(x, S, st).cpu().numpy()
            assert (mine == ref).all(), ("wrapper", kind, N, S, np.argwhere(mine != ref)[:3])
            for i, got in enumerate(_abi(dev, x, st, S, ws_bytes(S) if ws_bytes else None, twice)):
                assert (got == ref).all(), ("C ABI, call %d" % i, kind, N, S, np.argwhere(got != ref)[:3])


@pytest.mark.parametrize("N", [24577, 26625, 28672])
@pytest.mark.parametrize("rowmap", [0, 1, 2])
def test_fps_row_ownership_maps(dev, rowmap, N):
    """FPS_ROWMAP 0, 1, 2 (2 is the default): fps_rows_kernel<1024, PPT, ., MAP> at 25 / 28 points per thread -- a contiguous
    run of rows per wave, round robin, groups of four rows round robin (launch_fps_pruned: PPT >= FPS_ROWS_MIN_PPT = 24)."""
    with options(PN2_FPS_ROWMAP=rowmap):
        _check(dev, N, (64, 200))


@pytest.mark.parametrize("N", [8193, 16384, 20000, 22000])
def test_fps_rows_kernel_below_its_default_hand_over(dev, N):
    """FPS_ROWS_MIN_PPT = 16: the row-level pruned kernel at 16 / 20 / 22 points per thread, where the default runs the
    wave-level fps_pruned_kernel (launch_fps_pruned: `PPT >= 16` and `PPT >= rows_min`)."""
    with options(PN2_FPS_ROWS_MIN_PPT=16):
        _check(dev, N, (64, 200))


@pytest.mark.parametrize("N", [24577, 28672])
def test_fps_wave_level_pruned_kernel_above_its_default_hand_over(dev, N):
    """FPS_ROWS_MIN_PPT = 29: the wave-level fps_pruned_kernel<1024, 25 / 28> where the default runs the rows kernel."""
    with options(PN2_FPS_ROWS_MIN_PPT=29):
        _check(dev, N, (64, 200))


@pytest.mark.parametrize("N", [24577, 28672])
def test_fps_single_workgroup_kernel_at_28_points_per_thread(dev, N):
    """FPS_SINGLE_MAX = 28672 with FPS_PRUNE = 0: launch_fps<1024, 28> (pn2_fps: `N <= fps_single_max()` behind the pruned
    branch, which FPS_PRUNE = 0 closes), unreachable by default; no workspace."""
    with options(PN2_FPS_SINGLE_MAX=28672, PN2_FPS_PRUNE=0):
        _check(dev, N, (65,), ws_bytes=lambda S: 0)


def test_fps_three_workgroup_cooperative_plan(dev):
    """FPS_SINGLE_MAX = 16384: a 16 385-point cloud is cooperative (fps_coop_plan: 8 points per thread, W = 3 workgroups, the
    third holding one point); the workspace is the slot table, 32 bytes per cloud, sample and workgroup."""
    with options(PN2_FPS_SINGLE_MAX=16384):
        _check(dev, 16385, (8,), ws_bytes=lambda S: B * S * 3 * 32)


def test_fps_large_kernel_with_the_cooperative_plan_off(dev):
    """FPS_COOP = 0: fps_large_kernel (running distances in the workspace, B N floats) on two clouds, reached by default only
    when too many clouds oversubscribe the cooperative plan."""
    N = 24577
    with options(PN2_FPS_COOP=0):
        _check(dev, N, (6,), ws_bytes=lambda S: B * N * 4)


@pytest.mark.parametrize("N", [2049, 4096])
@pytest.mark.parametrize("piece", [1, 64, 100])
def test_fps_sampling_chain_in_pieces(dev, piece, N):
    """FPS_PIECE > 0 (2048 < N <= 4096): launch_fps_pieces -- the chain as launches of `piece` iterations, running distances and
    the current sample through the workspace (B (512 x 8 x 4 + 4) bytes, pn2_fps_workspace_bytes) -- at npoint = piece (pn2_fps:
    `npoint > piece` fails, the single launch), piece + 1, 2 piece and 2 piece + 1; the same call a second time on the dirty
    workspace must return the same indices."""
    with options(PN2_FPS_PIECE=piece):
        _check(dev, N, (piece, piece + 1, 2 * piece, 2 * piece + 1), ws_bytes=lambda S: B * (512 * 8 * 4 + 4), twice=True)


def test_zz_options_read_back_at_their_header_defaults(dev):
    """Every test above restores what it set: the library's options equal the defaults of PN2_OPTION_LIST (or what the
    environment of this process forwarded at load time)."""
    import os
    want = O.header_defaults()
    want.update({k: int(os.environ[k]) for k in want if k in os.environ})
    assert _lib.options() == want
