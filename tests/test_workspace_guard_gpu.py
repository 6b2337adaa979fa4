"""GPU: every entry point whose workspace is carved through ``Pn2Arena`` (csrc/pn2_common.h) stays inside the bytes its
``_workspace_bytes`` asks for, and reads nothing of the workspace that it did not write first.

Each call runs once at the smallest shape with a second tile and a ragged tail (1025 rows; device-side counts [1025, 0, 1] where
the entry point takes them).  Its workspace is a view of EXACTLY ``_workspace_bytes`` bytes, 16-byte (and not 256-byte) aligned,
inside a larger allocation with 4096 pattern bytes on either side, which must come back untouched.  Where include/pn2.h does not
ask the caller to initialise the workspace the call runs twice, the workspace prefilled with 0x00 and with 0xFF, and every output
is byte-equal; the two loss workspaces hold a ticket word that must be zero and run once.  With ``buffers=`` wrappers the
guarded view takes the place of ``buffers.workspace``; the others are called at the C ABI."""
import numpy as np
import pytest
import torch

import chamfer_ref

from pointnet12_amd import _lib, boxes, features, kitti, neighbors, plane, registration, voxel

pytestmark = pytest.mark.gpu

GUARD, PATTERN, SHIFT = 4096, 0xA5, 16
B, ROWS = 3, 1025
COUNTS = [1025, 0, 1]


class Guarded:
    """Hands out workspaces of exactly the bytes asked for, prefilled with ``fill``, each between two guards."""

    def __init__(self, dev, fill):
        self.dev, self.fill, self.held = dev, fill, []

    def take(self, nbytes):
        nbytes = int(nbytes)
        assert nbytes > 0
        hold = torch.full((SHIFT + GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=self.dev)
        view = hold[SHIFT + GUARD:SHIFT + GUARD + nbytes]
        view.fill_(self.fill)
        assert view.data_ptr() % 16 == 0 and view.data_ptr() % 256 != 0 and view.numel() == nbytes
        self.held.append((hold, nbytes))
        return view

    def intact(self):
        assert self.held, "the case took no workspace"
        for hold, nbytes in self.held:
            front, back = hold[:SHIFT + GUARD], hold[SHIFT + GUARD + nbytes:]
            assert back.numel() == GUARD
            assert bool((front == PATTERN).all()), "bytes BEFORE a workspace of %d bytes were written" % nbytes
            assert bool((back == PATTERN).all()), "bytes AFTER a workspace of %d bytes were written" % nbytes


def outputs_of(obj, skip=("workspace", "reduce_workspace", "table")):
    """The tensors a buffers object holds, but its workspaces and tables, by name."""
    return {k: v for k, v in vars(obj).items() if isinstance(v, torch.Tensor) and k not in skip}


def cleared(obj):
    """Zeroes every output of a buffers object: entries no launch writes then compare equal between two runs."""
    for t in outputs_of(obj).values():
        t.zero_()
    return obj


def as_bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def run_guarded(dev, case, fills=(0x00, 0xFF)):
    """Runs ``case(take) -> {name: tensor}`` once per prefill; guards intact, outputs written and byte-equal between the prefills."""
    seen = []
    for fill in fills:
        g = Guarded(dev, fill)
        out = case(g.take)
        torch.cuda.synchronize(dev)
        g.intact()
        seen.append({k: as_bytes(v) for k, v in out.items()})
        assert any(bool(v.any()) for v in seen[-1].values()), "the call wrote nothing"
    for other in seen[1:]:
        assert other.keys() == seen[0].keys()
        for k in other:
            assert torch.equal(other[k], seen[0][k]), "%s depends on what the workspace held before the call" % k


def ws_bytes(entry, *args):
    n = int(getattr(_lib.load(), entry)(*args))
    assert n > 0, (entry, args, n)
    return n


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def clouds(dev):
    """B clouds of ROWS rows back to back, [B * ROWS, 4] in a 4 m cube, with the device-side row ranges."""
    gen = torch.Generator(device="cpu").manual_seed(1025)
    pts = (torch.rand(B * ROWS, 4, generator=gen) * 4 - 2).to(dev)
    labels = torch.randint(0, 5, (B * ROWS,), generator=gen, dtype=torch.int32).to(dev)
    begin = (torch.arange(B, dtype=torch.int64) * ROWS).to(dev)
    count = torch.tensor(COUNTS, dtype=torch.int64, device=dev)
    return pts, labels, begin, count


def test_scan_filter(dev, clouds):
    pts, _, begin, count = clouds
    f = kitti.ScanFilter(None, subset="all", x_range=(-1.0, 1.0), device=dev)

    def case(take):
        buf = cleared(f.buffers(B * ROWS, B, ROWS))
        buf.workspace = take(ws_bytes("pn2_scan_filter_workspace_bytes", B, ROWS))
        f.filter(pts, None, begin, count, max_rows=ROWS, out=buf)
        return outputs_of(buf)
    run_guarded(dev, case)


def test_voxel_grid_and_components(dev, clouds):
    pts, labels, begin, count = clouds
    grid = voxel.VoxelGrid(0.5, device=dev)

    def case(take):
        buf = cleared(grid.buffers(B * ROWS, B, ROWS, 4))
        buf.workspace = take(ws_bytes("pn2_voxel_grid_workspace_bytes", B, ROWS))
        down = grid.downsample(pts, labels, begin, count, max_rows=ROWS, out=buf)
        comp = cleared(grid.component_buffers(B * ROWS, B, ROWS))
        comp.workspace = take(ws_bytes("pn2_voxel_components_workspace_bytes", B, ROWS))
        grid.components(pts, down, row_begin=begin, row_count=count, max_rows=ROWS, out=comp)
        out = outputs_of(buf)
        out.update(("component_" + k, v) for k, v in outputs_of(comp).items())
        return out
    run_guarded(dev, case)
    assert int(grid.error_flag.item()) == 0


def test_match_pairs(dev):
    gen = torch.Generator(device="cpu").manual_seed(7)
    M, D = 96, 8
    ft = torch.rand(B, M, D, generator=gen)
    fs = (ft[:, torch.randint(0, M, (ROWS,), generator=gen)] + 0.01 * torch.rand(B, ROWS, D, generator=gen)).to(dev)
    ft = ft.to(dev)
    n_source = torch.tensor(COUNTS, dtype=torch.int64, device=dev)

    def case(take):
        buf = cleared(features.match_buffers(ROWS, M, B, dev, mutual=False))
        buf.workspace = take(ws_bytes("pn2_match_pairs_workspace_bytes", B, ROWS))
        features.match_features(fs, ft, mutual=False, ratio=None, n_source=n_source, buffers=buf)
        return outputs_of(buf)
    run_guarded(dev, case)


def test_grid_build_and_query_self(dev, clouds):
    cand = clouds[0].view(B, ROWS, 4)
    index = neighbors.GridIndex(radius=0.4, device=dev)

    def case(take):
        buf = cleared(index.buffers(ROWS, B, k=4))
        buf.workspace = take(ws_bytes("pn2_grid_workspace_bytes", B, ROWS))
        index.build(cand, buffers=buf).query_self(4, return_dist=True, return_count=True, buffers=buf)
        return outputs_of(buf)
    run_guarded(dev, case)
    assert int(index.error_flag.item()) == 0


@pytest.mark.parametrize("C", [1, 16])
def test_segment_mean_and_mode(dev, clouds, C):
    _, labels, begin, count = clouds
    gen = torch.Generator(device="cpu").manual_seed(C)
    values = torch.rand(B * ROWS, C, generator=gen).to(dev)
    segments = 37
    inverse = torch.randint(0, segments, (B * ROWS,), generator=gen, dtype=torch.int32).to(dev)
    n_seg = torch.full((B,), segments, dtype=torch.int64, device=dev)
    nbytes = ws_bytes("pn2_segment_reduce_workspace_bytes", B, ROWS, C)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def case(take):
        mean = torch.zeros(B * ROWS, C, device=dev)
        n_out = torch.zeros(B * ROWS, dtype=torch.int32, device=dev)
        mode, votes = torch.zeros(B * ROWS, dtype=torch.int32, device=dev), torch.zeros(B * ROWS, dtype=torch.int32, device=dev)
        voxel.segment_mean(values, inverse, n_seg, row_begin=begin, row_count=count, max_rows=ROWS, out=mean, n_out=n_out,
                           error_flag=err, workspace=take(nbytes))
        voxel.segment_mode(labels, inverse, n_seg, return_votes=True, row_begin=begin, row_count=count, max_rows=ROWS, out=mode,
                           votes=votes, error_flag=err, workspace=take(ws_bytes("pn2_segment_reduce_workspace_bytes", B, ROWS, 1)))
        return dict(mean=mean, n_out=n_out, mode=mode, votes=votes)
    run_guarded(dev, case)
    assert int(err.item()) == 0


def test_lovasz_forward(dev):
    lib, images, C = _lib.load(), 2, 3
    R = images * ROWS
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(R, C, generator=gen).to(dev)
    target = torch.randint(0, C, (R,), generator=gen, dtype=torch.int64).to(dev)

    def case(take):
        ws = take(ws_bytes("pn2_lovasz_workspace_bytes", R, C, images))
        dp, loss = torch.zeros(R, C, device=dev), torch.zeros((), device=dev)
        _lib.check(lib.pn2_lovasz_fwd(x.data_ptr(), C, 0, target.data_ptr(), R, C, images, -100, 1, None, 1, ws.data_ptr(), dp.data_ptr(),
                                      None, loss.data_ptr(), _lib.stream()), "pn2_lovasz_fwd")
        return dict(dp=dp, loss=loss)
    run_guarded(dev, case)


def test_segment_boxes(dev, clouds):
    pts, _, begin, count = clouds
    gen = torch.Generator(device="cpu").manual_seed(11)
    segments = 9
    inverse = torch.randint(0, segments, (B * ROWS,), generator=gen, dtype=torch.int32).to(dev)
    n_seg = torch.full((B,), segments, dtype=torch.int64, device=dev)

    def case(take):
        buf = cleared(boxes.buffers(B * ROWS, B, ROWS, angles=4, device=dev))
        buf.angle.fill_(-1)
        buf.workspace = take(ws_bytes("pn2_segment_boxes_workspace_bytes", B, ROWS))
        boxes.segment_boxes(pts, inverse, n_seg, angles=4, row_begin=begin, row_count=count, max_rows=ROWS, buffers=buf)
        return outputs_of(buf)
    run_guarded(dev, case)


def test_fit_plane(dev, clouds):
    pts = clouds[0].view(B, ROWS, 4).clone()
    pts[:, ::2, 2] = 0.01 * pts[:, ::2, 3]                       # half of the rows within a centimetre of z = 0

    def case(take):
        buf = cleared(plane.buffers(ROWS, B, iterations=300, device=dev))
        buf.workspace = take(ws_bytes("pn2_plane_workspace_bytes", B, ROWS, 300))
        plane.fit_plane(pts, 0.05, iterations=300, seed=5, refine=1, buffers=buf)
        return outputs_of(buf)
    run_guarded(dev, case)


def test_correspondence_ransac(dev, clouds):
    src = clouds[0].view(B, ROWS, 4)[:, :, :3].contiguous()
    c, s = float(np.cos(0.3)), float(np.sin(0.3))
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device=dev)
    tgt = (src @ rot.T + torch.tensor([0.5, -0.25, 0.125], device=dev)).contiguous()
    pair = torch.arange(ROWS, dtype=torch.int64, device=dev).repeat(B, 1).contiguous()
    pair_tgt = pair.clone()
    pair_tgt[:, ::3] = pair_tgt[:, ::3].flip(1)                     # a third of the pairs are wrong

    def case(take):
        buf = cleared(registration.corr_buffers(ROWS, B, iterations=300, device=dev))
        buf.workspace = take(ws_bytes("pn2_corr_workspace_bytes", B, ROWS, 300))
        registration.ransac_correspondences(src, tgt, (pair, pair_tgt, None), 0.01, iterations=300, seed=9, refine=1, buffers=buf)
        return outputs_of(buf)
    run_guarded(dev, case)


def test_nll_and_cross_entropy_forward(dev):
    """(the ticket word of these two workspaces has to be zero: one run each, on a zeroed workspace)"""
    lib, R, C = _lib.load(), ROWS, 13
    gen = torch.Generator(device="cpu").manual_seed(13)
    x = torch.randn(R, C, generator=gen).to(dev)
    logp = torch.log_softmax(x, 1).contiguous()
    target = torch.randint(0, C, (R,), generator=gen, dtype=torch.int64).to(dev)

    def nll(take):
        ws = take(ws_bytes("pn2_nll_loss_workspace_bytes", R))
        res = torch.zeros(2, device=dev)
        _lib.check(lib.pn2_nll_loss_fwd(logp.data_ptr(), C, target.data_ptr(), None, R, C, -100, ws.data_ptr(), res.data_ptr(),
                                        res.data_ptr() + 4, _lib.stream()), "pn2_nll_loss_fwd")
        return dict(res=res)

    def cross_entropy(take):
        ws = take(ws_bytes("pn2_cross_entropy_workspace_bytes", R))
        res, lse = torch.zeros(2, device=dev), torch.zeros(R, device=dev)
        _lib.check(lib.pn2_cross_entropy_fwd(x.data_ptr(), C, 0, target.data_ptr(), None, R, C, -100, 0.0, 1, ws.data_ptr(), lse.data_ptr(),
                                             res.data_ptr(), res.data_ptr() + 4, _lib.stream()), "pn2_cross_entropy_fwd")
        return dict(res=res, lse=lse)
    run_guarded(dev, nll, fills=(0x00,))
    run_guarded(dev, cross_entropy, fills=(0x00,))


def test_chamfer_smallest_join(dev):
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    (Bc, N, M, D), = [shape for name, shape, _ in chamfer_ref.cases(cus) if name == "smallest-join"]
    assert chamfer_ref.plan(Bc, N, M, cus)[2] > 1                   # (split candidates: the workspace has all three parts)
    p1, p2 = (t.to(dev) for t in chamfer_ref.seeded(5, Bc, N, M, D))

    def case(take):
        ws = take(ws_bytes("pn2_chamfer_nn_workspace_bytes", Bc, N, M, D))
        dist, idx, total = torch.zeros(Bc, N, device=dev), torch.zeros(Bc, N, dtype=torch.int64, device=dev), torch.zeros((), device=dev)
        _lib.check(lib.pn2_chamfer_nn(p1.data_ptr(), p2.data_ptr(), Bc, N, M, D, dist.data_ptr(), idx.data_ptr(), total.data_ptr(),
                                      ws.data_ptr(), _lib.stream()), "pn2_chamfer_nn")
        return dict(dist=dist, idx=idx, total=total)
    run_guarded(dev, case)
