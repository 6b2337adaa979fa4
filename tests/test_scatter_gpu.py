"""GPU: the index-driven kernels (csrc/gather.hip, csrc/scatter.hip, the factorised first layer of csrc/grouped.hip), each
called through the C ABI and held to the fp64 statements of tests/scatter_ref.py.

Scattered sums (dP2, G, grad_points) are checked per element against ``scatter_ref.bound`` -- 1.05 (n + 4) 2^-24 A, derived
there, not measured -- with elements that receive no term exactly 0; on the exactly summable data of scatter_ref they must
be BIT-equal to the fp64 sum (-0 and +0 taken as equal), which is what sees one dropped, doubled or misplaced member.
Forward gathers and the interpolation forward are bit-equal to the oracle / the separately rounded float32 statement.

Coverage of the two segmented kernels by construction (every listed combination runs in a passing case):

    pn2_three_interp_bwd_seg   test_interp_bwd_constructed[D-layout], every case with PN2_SEG_CHUNK = 16, 32, 64, some also 0 (automatic)
        lpr_log2   0: D 1, 3, 4   1: D 5   2: D 16   3: D 17   4: D 64   5: D 100, 128   6: D 256, 260, 1024 (column loop)
        loads      "vec":    (ld, col0) = (320 + round4(D) + 4, 320): float4 where c + 3 < D, scalar tail elsewhere
                   "scalar": (ld, col0) = (round4(22 + D), 22)
    pn2_group_affine_bwd_seg   test_group_affine_bwd_constructed[C], the same four chunk settings, with and without dwx_scratch
        lpr_log2   0: C 4   1: C 6   2: C 16   3: C 32   4: C 48, 50, 64   5: C 96, 128   6: C 256   (always float4 loads)

Segment shapes per chunk length c (scatter_ref.constructed_cases, each run with each c): length c (ends on a chunk edge),
c + 1 and c - 1 (straddle one edge, drifting through every offset), 1, one owner for a whole cloud (whole chunks of one
owner), three targets, mostly empty targets, member counts of 1365 (not a multiple of 4 nor of a chunk, so the cloud's
last chunk is short), and for the segmented kernels a tail of dropped entries.

Not tested: group_kernel<uint64_t> (the 64-bit index arithmetic of pn2_group, taken from 2^32 float4s of output = 64 GiB).
The atomic kernels and the two forward kernels index without a range check and get in-range indices only.

dWx sums all B*S*K rows, so the a-priori bound says nothing (n ~ 1e6); it is held to max(3e-6 max|ref|, 4 x the error of the
same contraction in plain torch fp32), the rule tests/test_mlp_gpu.py uses for sums over all rows.  Measured: see
``_check_dwx``.

Both implementations of pn2_invert_index write -1 into the slots of dropped entries of members AND owners
(test_invert_index_members_and_owners; the three-pass path used to leave that tail of owners unwritten).

The fp64 references are formed on the GPU and the runs of one problem are checked together (one synchronisation), so the
file takes 5.5 s on an MI355X, next to 6.0 s for tests/test_geometry_gpu.py.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import scatter_ref as R
from oracle import geometry as G
from pointnet12_amd import _lib
from pointnet12_amd import pointnet_util as U
from pointnet12_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                        # a quiet-NaN bit pattern no kernel produces
GARBAGE = 0x5A5A5A5A
PN2_EINVAL = -1                          # include/pn2.h
I32 = torch.int32
CHUNK_SETTINGS = R.CHUNKS + (0,)         # forced 16 / 32 / 64 and the automatic choice
AUTO_ALSO = ("len1", "len33", "three_targets")   # constructed cases that run the automatic choice besides the three forced ones


def chunk_settings(name):
    return CHUNK_SETTINGS if (name in AUTO_ALSO or not name.startswith(("len", "one_owner", "mostly_empty"))) else R.CHUNKS


def r4(c):
    return (c + 3) & ~3


def lib_st():
    return _lib.load(), torch.cuda.current_stream().cuda_stream


def sentinel(shape, dev):
    return torch.full(shape, SENT, dtype=I32, device=dev).view(torch.float32)


def is_sent(t):
    return t.contiguous().view(I32) == SENT


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


def same_sum_bits(out, ref64):
    """Bit equality of a sum with the fp64 reference cast to float32, -0 and +0 taken as equal (x + 0 maps -0 to +0)."""
    return torch.equal((out + 0.0).contiguous().view(I32), (ref64.float() + 0.0).contiguous().view(I32))


@contextlib.contextmanager
def seg_chunk(value):
    old = _lib.options()["PN2_SEG_CHUNK"]
    _lib.set_option("PN2_SEG_CHUNK", value)
    try:
        yield
    finally:
        _lib.set_option("PN2_SEG_CHUNK", old)


def invert(idx2d, T):
    """pn2_invert_index on buffers pre-filled with garbage (the library must write every slot it promises)."""
    lib, st = lib_st()
    B, M = idx2d.shape
    assert idx2d.dtype == torch.int64 and idx2d.is_contiguous() and idx2d.is_cuda
    members = torch.full((B, M), GARBAGE, dtype=I32, device=idx2d.device)
    owners = torch.full((B, M), GARBAGE, dtype=I32, device=idx2d.device)
    scratch = torch.empty(B, 2 * T + 1, dtype=I32, device=idx2d.device)
    assert lib.pn2_invert_index(idx2d.data_ptr(), B, M, T, members.data_ptr(), owners.data_ptr(), scratch.data_ptr(), st) == 0
    return members, owners


def check_sums(outs, ref, n, A):
    """outs: [(tag, tensor)] of one problem, checked together (one device synchronisation for all of them): per element
    |out - ref| <= bound(n, A), and an element without a term exactly 0 -> worst error / bound."""
    stack = torch.stack([o for _, o in outs])
    err = (stack.double() - ref).abs()
    b = R.bound(n.unsqueeze(-1), A)
    outside = (err > b).flatten(1).sum(1)
    nonzero_empty = ((stack != 0) & (n == 0).unsqueeze(-1)).flatten(1).sum(1)
    ratio = (err / b.clamp_min(1e-300)).flatten(1).amax(1)
    outside, nonzero_empty, ratio = torch.stack([outside.double(), nonzero_empty.double(), ratio]).cpu()
    for i, (tag, _) in enumerate(outs):
        assert int(outside[i]) == 0, (tag, "worst error / bound", float(ratio[i]), "elements outside", int(outside[i]))
        assert int(nonzero_empty[i]) == 0, (tag, "elements without members that are not 0", int(nonzero_empty[i]))
    return float(ratio.max())


def check_sum(out, ref, n, A, tag):
    return check_sums([(tag, out)], ref, n, A)


def check_exacts(outs, ref, A, unit):
    """outs: [(tag, tensor)] of one problem on exactly summable data: each bit-equal to the fp64 sum cast to float32."""
    R.assert_exactly_summable(A, unit)
    stack = torch.stack([o for _, o in outs])
    differing = ((stack + 0.0).view(I32) != (ref.float() + 0.0).contiguous().view(I32)).flatten(1).sum(1).cpu()
    for i, (tag, _) in enumerate(outs):
        assert int(differing[i]) == 0, (tag, "not bit-equal on exactly summable data: elements differing", int(differing[i]))
    return 0.0


def check_exact(out, ref, A, unit, tag):
    check_exacts([(tag, out)], ref, A, unit)


@functools.lru_cache(maxsize=None)
def _level(B, n0, N, S, seed):
    """KITTI-shaped clouds of n0 points -> (xyz of the level's N points, xyz of its S centres), by farthest point sampling."""
    pts, _ = syn.kitti_batch(seed, B, n0)
    xyz = torch.from_numpy(np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))).cuda()

    def sub(x, n):
        if n == x.shape[1]:
            return x
        fps = U.farthest_point_sample(x, n, torch.zeros(B, dtype=torch.int64))
        return U.index_points(x, fps).detach().contiguous()
    xn = sub(xyz, N)
    return xn, sub(xn, S)


_cases = functools.lru_cache(maxsize=None)(R.constructed_cases)      # (the same indices for every channel count)


# ------------------------------------------------------------------------------------------ pn2_three_interp (forward)

@pytest.mark.parametrize("col0", [0, 22, 320])
@pytest.mark.parametrize("D", [1, 3, 63, 64, 65, 128, 1024])
def test_three_interp_forward_bit_equal(dev, D, col0):
    """Bit-equal to ((p0*w0 + p1*w1) + p2*w2) in separately rounded float32, written at col0 of a sentinel-filled row: with
    zero_tail the columns right of col0 + D are 0, without it they keep the sentinel; the columns left of col0 are the copy
    of points1 or keep the sentinel."""
    lib, st = lib_st()
    B, N, S = 2, 301, 50
    g = torch.Generator(device=dev).manual_seed(1000 * D + col0)
    p2 = torch.randn(B, S, D, device=dev, generator=g)
    idx = torch.randint(0, S, (B, N, 3), device=dev, generator=g)
    w = torch.rand(B, N, 3, device=dev, generator=g) + 1e-3
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    ref = R.interp_fwd(p2, idx, w).view(B * N, D)
    p1 = torch.randn(B, N, col0, device=dev, generator=g) if col0 else None
    for ld in (col0 + D, col0 + D + 5):
        for use_p1 in ((False, True) if col0 else (False,)):
            for zero_tail in (0, 1):
                out = sentinel((B * N, ld), dev)
                assert lib.pn2_three_interp(p2.data_ptr(), idx.data_ptr(), w.data_ptr(), B, N, S, D, out.data_ptr(), ld, col0,
                                            zero_tail, p1.data_ptr() if use_p1 else None, st) == 0
                tag = (ld, use_p1, zero_tail)
                assert bits_equal(out[:, col0:col0 + D], ref), tag
                left, right = out[:, :col0], out[:, col0 + D:]
                if use_p1:
                    assert bits_equal(left, p1.view(B * N, col0)), tag
                else:
                    assert bool(is_sent(left).all()), tag
                if zero_tail:
                    assert bool((right.contiguous().view(I32) == 0).all()), tag
                    if use_p1 or col0 == 0:
                        assert not bool(is_sent(out).any()), tag
                else:
                    assert bool(is_sent(right).all()), tag


# ----------------------------------------------------------------------------------------- pn2_three_interp_bwd[_seg]

INTERP_D = [1, 3, 4, 5, 16, 17, 64, 100, 128, 256, 260, 1024]


def _interp_layout(D, layout):
    """(ld, col0): "vec" = both multiples of 4 (float4 loads), "scalar" = col0 22 under a multiple-of-4 pitch."""
    return (320 + r4(D) + 4, 320) if layout == "vec" else (r4(22 + D), 22)


def _interp_bwd_atomic(grad, ld, col0, D, idx3, w, S):
    lib, st = lib_st()
    B, N, _ = idx3.shape
    out = torch.zeros(B, S, D, device=grad.device)
    assert lib.pn2_three_interp_bwd(grad.data_ptr(), ld, col0, idx3.data_ptr(), w.data_ptr(), B, N, S, D, out.data_ptr(), st) == 0
    return out


def _interp_bwd_seg(grad, ld, col0, D, mem, own, w, S):
    lib, st = lib_st()
    B, N = w.shape[:2]
    out = torch.zeros(B, S, D, device=grad.device)
    assert lib.pn2_three_interp_bwd_seg(grad.data_ptr(), ld, col0, mem.data_ptr(), own.data_ptr(), w.data_ptr(), B, N, S, D,
                                        out.data_ptr(), st) == 0
    return out


def _interp_data(B, N, ld, seed, dev, w_random=None):
    """(grad [2B,N,ld], w [2B,N,3]): clouds 0..B-1 carry random data (weights w_random if given), clouds B..2B-1 the exactly
    summable data -- clouds are independent, so one launch over 2B clouds checks both."""
    gr, wr = R.random_interp_data(B, N, ld, seed, dev)
    ge, we = R.exact_interp_data(B, N, ld, seed + 1, dev)
    return torch.cat([gr, ge]).contiguous(), torch.cat([wr if w_random is None else w_random, we]).contiguous()


def _check_interp_bwd(dev, name, idx2d, T, N, D, ld, col0, data, atomic):
    """One index [B, 3N] on both data sets at once (2B clouds, the index repeated): the atomic kernel (in-range indices
    only) and the segmented kernel with every chunk setting; the random half within the bound, the exactly summable half
    bit-equal -> worst error / bound seen on the random half."""
    B = idx2d.shape[0]
    grad, w = data
    idx_d = torch.cat([idx2d, idx2d]).to(dev).contiguous()
    idx3 = idx_d.view(2 * B, N, 3)
    mem, own = invert(idx_d, T)
    ref, n, A = R.interp_bwd(grad, col0, D, idx3, w, T)
    outs = []
    if atomic:
        outs.append(((name, "atomic"), _interp_bwd_atomic(grad, ld, col0, D, idx3, w, T)))
    for chunk in chunk_settings(name):
        with seg_chunk(chunk):
            outs.append(((name, "seg", chunk), _interp_bwd_seg(grad, ld, col0, D, mem, own, w, T)))
    check_exacts([(t + ("exact",), o[B:]) for t, o in outs], ref[B:], A[B:], R.EXACT_INTERP_UNIT)
    return check_sums([(t + ("random",), o[:B]) for t, o in outs], ref[:B], n[:B], A[:B])


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("D", INTERP_D)
def test_interp_bwd_constructed(dev, D, layout):
    """pn2_three_interp_bwd (atomics) and pn2_three_interp_bwd_seg (chunks 16 / 32 / 64 / automatic) on every constructed
    index of scatter_ref, random data within the derived bound and exactly summable data bit-equal; the segmented kernel
    also with a tenth of the entries out of range (dropped)."""
    B, N = 3, 455                                          # 1365 members per cloud: the last chunk of a cloud is short
    ld, col0 = _interp_layout(D, layout)
    assert (((ld | col0) & 3) == 0) == (layout == "vec")
    data = _interp_data(B, N, ld, D, dev)
    worst = 0.0
    for name, idx, T in _cases(3 * N, 100, B):
        worst = max(worst, _check_interp_bwd(dev, name, idx, T, N, D, ld, col0, data, atomic=True))
        if name in ("len17", "len32", "len63", "three_targets"):
            worst = max(worst, _check_interp_bwd(dev, name + "_dropped", R.with_dropped(idx, T, D), T, N, D, ld, col0, data,
                                                 atomic=False))
    print("interp_bwd D=%d %s: worst error / bound %.3f" % (D, layout, worst))


@pytest.mark.parametrize("N", [1, 5, 21])
def test_interp_bwd_tiny_clouds(dev, N):
    """3, 15 and 63 members: a cloud shorter than one chunk, member counts that are not a multiple of 4."""
    B = 3
    for D, layout in ((3, "scalar"), (4, "vec"), (65, "vec")):
        ld, col0 = _interp_layout(D, layout)
        data = _interp_data(B, N, ld, N, dev)
        for T in (3, 7, 200):
            _check_interp_bwd(dev, "T%d" % T, R.random_index(B, 3 * N, T, N + T), T, N, D, ld, col0, data, atomic=True)


@pytest.mark.parametrize("N,length", [(65536, 196608), (333334, 15), (333334, 33), (333334, 64)])
def test_interp_bwd_seg_long_lists(dev, N, length):
    """One target owning a whole cloud of 196 608 members (the bound is blind there: the exactly summable data decides),
    and 1 000 002 members per cloud (not a multiple of any chunk) in segments around the chunk lengths."""
    B, M = 2, 3 * N
    T = -(-M // length) + 7
    idx = R.segments_index(B, M, T, length, N + length)
    for D, ld, col0 in ((4, 4, 0), (3, 5, 1)):                 # float4 and scalar loads
        worst = _check_interp_bwd(dev, "long%d" % length, idx, T, N, D, ld, col0, _interp_data(B, N, ld, N, dev), atomic=(length < 100))
        print("interp_bwd N=%d segments of %d, D=%d: worst error / bound %.4f" % (N, length, D, worst))


@pytest.mark.parametrize("level", ["msg_fp1", "msg_fp2", "ssg_fp4", "cfg5_fp1"])
def test_interp_bwd_real_geometry(dev, level):
    """The 3-NN index of KITTI-shaped clouds at the product's level sizes (scalar loads at fp1: ld 140, col0 9; float4 at
    fp2 / fp4; D2 = 512 loops the column block)."""
    B, n0, N, S, D, ld, col0 = {"msg_fp1": (16, 4096, 4096, 512, 128, 140, 9), "msg_fp2": (16, 4096, 512, 128, 256, 576, 320),
                                "ssg_fp4": (16, 4096, 64, 16, 512, 768, 256), "cfg5_fp1": (2, 65536, 65536, 8192, 128, 140, 9)}[level]
    xn, xs = _level(B, n0, N, S, 40)
    idx3, _, w_real = U.three_nn(xn, xs)
    assert int(idx3.min()) >= 0 and int(idx3.max()) < S
    worst = _check_interp_bwd(dev, level, idx3.reshape(B, 3 * N).cpu(), S, N, D, ld, col0, _interp_data(B, N, ld, 7, dev, w_real), atomic=True)
    print("interp_bwd %s: worst error / bound %.3f" % (level, worst))


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("D", [1, 3, 64, 65, 260, 1024])
def test_interp_bwd_single_target(dev, D, layout):
    """S == 1: three_interp_bwd_single_kernel, a column sum that is STORED (a sentinel-filled output ends without one) and
    identical from run to run; the segmented kernel on the same problem (T = 1 through pn2_invert_index)."""
    lib, st = lib_st()
    B = 3
    ld, col0 = _interp_layout(D, layout)
    for N in (1, 5, 128, 455):
        idx3 = torch.zeros(B, N, 3, dtype=torch.int64, device=dev)
        mem, own = invert(idx3.view(B, 3 * N), 1)
        for kind, (grad, w) in (("random", R.random_interp_data(B, N, ld, D + N, dev)), ("exact", R.exact_interp_data(B, N, ld, D + N, dev))):
            ref, n, A = R.interp_bwd(grad, col0, D, idx3, w, 1)
            outs = []
            for _ in range(2):
                out = sentinel((B, 1, D), dev)
                assert lib.pn2_three_interp_bwd(grad.data_ptr(), ld, col0, idx3.data_ptr(), w.data_ptr(), B, N, 1, D, out.data_ptr(), st) == 0
                assert not bool(is_sent(out).any())
                outs.append(out)
            assert bits_equal(outs[0], outs[1])
            with seg_chunk(16):
                outs.append(_interp_bwd_seg(grad, ld, col0, D, mem, own, w, 1))
            for out in outs[1:]:
                if kind == "exact":
                    check_exact(out, ref, A, R.EXACT_INTERP_UNIT, (N, kind))
                else:
                    check_sum(out, ref, n, A, (N, kind))


# ----------------------------------------------------------------- pn2_gather_rows[_bwd], pn2_group[_bwd], pn2_copy_cols

def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("C", [1, 3, 6, 9, 61, 64, 125])
def test_gather_rows_forward_and_backward(dev, C):
    lib, st = lib_st()
    B, N, M = 2, 100, 77
    g = torch.Generator(device=dev).manual_seed(C)
    pts = torch.randn(B, N, C, device=dev, generator=g)
    idx = torch.randint(0, N, (B, M), device=dev, generator=g)
    bad = idx.clone()
    bad[0, 3], bad[1, 0], bad[1, M - 1] = -1, N, N + 3
    for ix, has_bad in ((idx, False), (bad, True)):
        out, err = sentinel((B, M, C), dev), torch.zeros(1, dtype=I32, device=dev)
        assert lib.pn2_gather_rows(pts.data_ptr(), ix.data_ptr(), B, N, C, M, out.data_ptr(), err.data_ptr(), st) == 0
        ok = (ix >= 0) & (ix < N)
        ref = torch.from_numpy(G.index_points(_np(pts), _np(torch.where(ok, ix, torch.zeros_like(ix))))).to(dev)
        ref[~ok] = 0.0                                          # out-of-range rows are written as zeros
        assert bits_equal(out, ref) and int(err.item()) == int(has_bad)
    for kind in ("random", "exact"):
        grad = torch.randn(B, M, C, device=dev, generator=g) if kind == "random" else torch.randint(-8, 9, (B, M, C), device=dev, generator=g).float()
        gp = torch.zeros(B, N, C, device=dev)
        assert lib.pn2_gather_rows_bwd(grad.data_ptr(), bad.data_ptr(), B, N, C, M, gp.data_ptr(), st) == 0
        ref, n, A = R.gather_rows_bwd(grad, bad, N)
        assert float(n.sum()) == B * M - 3
        check_sum(gp, ref, n, A, kind) if kind == "random" else check_exact(gp, ref, A, 1.0, kind)


@pytest.mark.parametrize("xyz_first", [0, 1])
@pytest.mark.parametrize("D", [0, 1, 3, 6, 9, 61, 64, 125])
def test_group_forward_and_backward(dev, D, xyz_first):
    """pn2_group bit-equal to the oracle on a sentinel-filled output (every element written, pad columns 0, out-of-range rows
    0 with err set), new_xyz == NULL, idx == NULL with K == N; pn2_group_bwd within the bound, indices equal to N dropped."""
    lib, st = lib_st()
    B, N, S = 2, 50, 7
    g = torch.Generator(device=dev).manual_seed(10 * D + xyz_first)
    xyz, ctr = torch.randn(B, N, 3, device=dev, generator=g), torch.randn(B, S, 3, device=dev, generator=g)
    pts = torch.randn(B, N, D, device=dev, generator=g) if D else None
    for K, use_idx, centred, ld in ((5, True, True, r4(3 + D)), (5, True, False, r4(3 + D) + 4), (N, False, True, r4(3 + D))):
        idx = torch.randint(0, N, (B, S, K), device=dev, generator=g) if use_idx else None
        bad = None
        if use_idx:
            bad = idx.clone()
            bad[0, 1, 2], bad[1, S - 1, K - 1], bad[1, 0, 0] = N, N, -1
        P = B * S * K
        for ix in ((idx, bad) if use_idx else (None,)):
            out, err = sentinel((P, ld), dev), torch.zeros(1, dtype=I32, device=dev)
            assert lib.pn2_group(xyz.data_ptr(), pts.data_ptr() if D else None, ctr.data_ptr() if centred else None,
                                 ix.data_ptr() if use_idx else None, B, N, S, K, D, xyz_first, ld, out.data_ptr(), err.data_ptr(), st) == 0
            full = ix if use_idx else torch.arange(K, device=dev).expand(B, S, K)
            ok = (full >= 0) & (full < N)
            ref = G.group(_np(xyz), _np(pts) if D else None, _np(ctr) if centred else np.zeros((B, S, 3), np.float32),
                          _np(torch.where(ok, full, torch.zeros_like(full))), xyz_first, ld)
            ref = torch.from_numpy(ref).to(dev).view(P, ld)
            ref[~ok.reshape(-1)] = 0.0
            assert bits_equal(out, ref), (K, use_idx, centred)
            assert bool((out[:, 3 + D:].contiguous().view(I32) == 0).all())
            assert int(err.item()) == int(not bool(ok.all()))
        if D == 0:
            continue
        for kind in ("random", "exact"):
            rows = torch.randn(P, ld, device=dev, generator=g) if kind == "random" else torch.randint(-8, 9, (P, ld), device=dev, generator=g).float()
            gp = torch.zeros(B, N, D, device=dev)
            assert lib.pn2_group_bwd(rows.data_ptr(), bad.data_ptr() if use_idx else None, B, N, S, K, D, xyz_first, ld,
                                     gp.data_ptr(), st) == 0
            ref, n, A = R.group_bwd(rows, bad, B, N, S, K, D, xyz_first)
            check_sum(gp, ref, n, A, (K, kind)) if kind == "random" else check_exact(gp, ref, A, 1.0, (K, kind))


def test_copy_cols_bit_equal_with_untouched_surroundings(dev):
    lib, st = lib_st()
    for rows, cols, lds, scol0, ldd, dcol0 in ((1, 1, 1, 0, 1, 0), (37, 5, 9, 3, 12, 7), (1000, 128, 140, 9, 128, 0), (513, 320, 320, 0, 576, 0),
                                               (64, 3, 131, 128, 3, 0)):
        src = torch.randn(rows, lds, device=dev)
        dst = sentinel((rows, ldd), dev)
        assert lib.pn2_copy_cols(src.data_ptr(), lds, scol0, dst.data_ptr(), ldd, dcol0, rows, cols, st) == 0
        assert bits_equal(dst[:, dcol0:dcol0 + cols], src[:, scol0:scol0 + cols])
        assert bool(is_sent(dst[:, :dcol0]).all()) and bool(is_sent(dst[:, dcol0 + cols:]).all())


# ------------------------------------------------------------------------------------------------ pn2_group_affine_fwd

def _affine_fwd(dev, B, N, S, K, C, idx3, xyz, ctr, full_weight, seed):
    lib, st = lib_st()
    P, C4 = B * S * K, r4(C)
    g = torch.Generator(device=dev).manual_seed(seed)
    ldz, ldy, Dw = C4 + (4 if full_weight else 0), C4 + 4, (5 if full_weight else 0)
    Zf = torch.randn(B * N, ldz, device=dev, generator=g)
    W = torch.randn(C, 3 + Dw, device=dev, generator=g) * 0.3        # [features, xyz]: Wx points into the full weight
    Wx = W[:, Dw:]
    Yref, mag, s0, s1 = R.group_affine_fwd(Zf[:, :C], xyz, ctr, idx3, Wx)
    outs = []
    for with_stats in (True, False):
        Y = sentinel((P, ldy), dev)
        stats = torch.zeros(8 * 2 * C, dtype=torch.float64, device=dev)          # PN2_STAT_REPLICAS copies
        assert lib.pn2_group_affine_fwd(Zf.data_ptr(), ldz, xyz.data_ptr(), ctr.data_ptr(), idx3.data_ptr(), W.data_ptr() + 4 * Dw, 3 + Dw,
                                        B, N, S, K, C, Y.data_ptr(), ldy, stats.data_ptr() if with_stats else None, st) == 0
        outs.append(Y)
        err = (Y[:, :C].double() - Yref).abs()
        tol = 5 * R.U32 * mag                          # one rounded difference and three fmas (shown valid in test_scatter_ref_cpu.py)
        assert bool((err <= tol).all()), (C, float((err / tol.clamp_min(1e-300)).max()))
        assert bool((Y[:, C:C4].contiguous().view(I32) == 0).all()) and bool(is_sent(Y[:, C4:]).all())
        if with_stats:
            st_ = stats.view(8, 2, C).sum(0)
            mean, var = st_[0] / P, st_[1] / P - (st_[0] / P) ** 2
            rmean = s0 / P
            assert torch.allclose(mean, rmean, rtol=1e-5, atol=1e-6)             # the bound of tests/test_mlp_gpu.py::_check_shared_mlp
            assert torch.allclose(var, s1 / P - rmean ** 2, rtol=1e-5, atol=1e-6)
    assert bits_equal(outs[0], outs[1])
    return float((err / tol.clamp_min(1e-300)).max())


@pytest.mark.parametrize("full_weight", [False, True])
@pytest.mark.parametrize("C", [4, 32, 48, 50, 64, 96, 128, 256, 1024])
def test_group_affine_forward(dev, C, full_weight):
    B, N, S, K = 2, 200, 32, 16
    g = torch.Generator(device=dev).manual_seed(C)
    xyz, ctr = torch.rand(B, N, 3, device=dev, generator=g) * 2 - 1, torch.rand(B, S, 3, device=dev, generator=g) * 2 - 1
    idx3 = R.random_index(B, S * K, N, C).view(B, S, K).to(dev)
    _affine_fwd(dev, B, N, S, K, C, idx3, xyz, ctr, full_weight, C + 1)


def test_group_affine_forward_benchmark_level(dev):
    """cfg5's sa2 (B = 2: 524 288 grouped rows, C = 128): the grid is capped, every thread walks 64 rows and folds its fp32
    statistics into fp64 on the way."""
    B, N, S, K, C = 2, 8192, 2048, 128, 128
    xn, xs = _level(B, 65536, N, S, 40)
    idx3 = U.query_ball_point(0.8, K, xn, xs)
    assert int(idx3.min()) >= 0 and int(idx3.max()) < N
    print("affine_fwd cfg5 sa2: worst error / bound %.3f" % _affine_fwd(dev, B, N, S, K, C, idx3, xn, xs, True, 3))


# --------------------------------------------------------------------------------------- pn2_group_affine_bwd[_seg]

def _coef_block(coef, C, dev):
    C4 = r4(C)
    blk = torch.zeros(4 * C4, device=dev)
    for i in range(4):
        blk[i * C4:i * C4 + C] = coef[i]
    return blk


def _padded(t, ld, seed):
    """[P, C] -> [P, ld] with finite random pad columns (a zero coefficient pad must still give a zero G pad)."""
    out = torch.randn(t.shape[0], ld, device=t.device, generator=torch.Generator(device=t.device).manual_seed(seed))
    out[:, :t.shape[1]] = t
    return out


def _check_dwx(kind, runs, start, Dw, ref, AW, dY32, rel32):
    """runs: [(tag, dW)], the sentinel-surrounded weight gradients of one problem; their xyz columns must hold start + dWx
    and their feature columns the sentinel.  Exactly summable data: bit-equal.  Random data: within
    max(3e-6 max|ref|, 4 x yardstick), yardstick = |dY32^T rel32 - ref| of plain torch fp32 on the GPU.
    Measured on an MI355X, relative to max|ref| (printed per test with -s): constructed indices (4 089 rows) kernels
    5e-8 .. 7.7e-7, yardstick 2.8e-7 .. 1.4e-6; product level sizes and the grid-stride case (16 384 .. 524 288 rows)
    kernels 1.2e-7 .. 1.1e-6, yardstick 6.8e-7 .. 2.9e-6.
    -> [(kernel error, yardstick error)] relative to max|ref| (random data)."""
    stack = torch.stack([dW for _, dW in runs])
    written = (~is_sent(stack[:, :, :Dw])).flatten(1).sum(1)
    if kind == "exact":
        R.assert_exactly_summable(AW + start.double().abs(), R.EXACT_AFFINE_UNIT_DWX)
        want = (start.double() + ref).float() + 0.0
        differing = ((stack[:, :, Dw:] + 0.0).contiguous().view(I32) != want.contiguous().view(I32)).flatten(1).sum(1)
        written, differing = torch.stack([written, differing]).cpu()
        for i, (tag, _) in enumerate(runs):
            assert int(written[i]) == 0, (tag, "feature columns of the weight gradient were written")
            assert int(differing[i]) == 0, (tag, "dWx not bit-equal on exactly summable data", int(differing[i]))
        return []
    err = ((stack[:, :, Dw:] - start).double() - ref).abs().flatten(1).amax(1)
    yard = ((dY32.t() @ rel32).double() - ref).abs().max()
    vals = torch.cat([written.double(), err, yard.view(1), ref.abs().max().view(1)]).cpu()
    k, (yard, scale) = len(runs), (float(vals[-2]), float(vals[-1]))
    for i, (tag, _) in enumerate(runs):
        assert int(vals[i]) == 0, (tag, "feature columns of the weight gradient were written")
        assert float(vals[k + i]) <= max(3e-6 * scale, 4 * yard), (tag, float(vals[k + i]) / scale, yard / scale)
    return [(float(vals[k + i]) / scale, yard / scale) for i in range(k)]


def _affine_bwd_case(dev, name, idx2d, B, N, S, K, C, seed, atomic, chunks=None, kinds=("random", "exact")):
    """One index, both data sets: pn2_group_affine_bwd (in-range indices only) and pn2_group_affine_bwd_seg with every chunk
    setting, alternately with and without dwx_scratch -> [(kernel error, yardstick error) of dWx relative to max|ref|]."""
    lib, st = lib_st()
    chunks = chunks or chunk_settings(name)
    P, C4, Dw = B * S * K, r4(C), 6
    ldz, ldy, ldg = C4 + 4, C4, C4 + 4
    idx3 = idx2d.to(dev).contiguous().view(B, S, K)
    mem, own = invert(idx3.view(B, S * K), N)
    seen = []
    for kind in kinds:
        dZ, Y, coef, xyz, ctr = (R.random_affine_data if kind == "random" else R.exact_affine_data)(B, N, S, K, C, seed, dev)
        dY, Gref, n, A, Wref, AW = R.group_affine_bwd(dZ, Y, coef, xyz, ctr, idx3)
        valid = ((idx3 >= 0) & (idx3 < N)).reshape(-1, 1)
        rel32 = (xyz.reshape(-1, 3)[(idx3.clamp(0, N - 1) + torch.arange(B, device=dev).view(B, 1, 1) * N).reshape(-1)].view(B, S, K, 3)
                 - ctr.unsqueeze(2)).reshape(-1, 3)
        dY32 = (coef[0] * dZ + (coef[1] * (Y - coef[3]) + coef[2])) * valid
        dZp, Yp, blk = _padded(dZ, ldz, 1), _padded(Y, ldy, 2), _coef_block(coef, C, dev)
        g = torch.Generator(device=dev).manual_seed(seed + 5)
        start = torch.randn(C, 3, device=dev, generator=g) if kind == "random" else torch.randint(-3, 4, (C, 3), device=dev, generator=g).float()
        settings = [None] if atomic else []                      # None: the atomic kernel; else (chunk, with dwx_scratch)
        if C <= 256:
            for i, chunk in enumerate(chunks):
                settings += [(chunk, scratch) for scratch in ((False, True) if i == 0 else (bool(i & 1),))]
        Gs, dWs = [], []
        for setting in settings:
            Gm = torch.zeros(B * N, ldg, device=dev)
            dW = sentinel((C, Dw + 3), dev)
            dW[:, Dw:] = start
            common = (dZp.data_ptr(), ldz, Yp.data_ptr(), ldy, blk.data_ptr(), xyz.data_ptr(), ctr.data_ptr())
            if setting is None:
                rc = lib.pn2_group_affine_bwd(*common, idx3.data_ptr(), B, N, S, K, C, Gm.data_ptr(), ldg, dW.data_ptr() + 4 * Dw, Dw + 3, st)
            else:
                chunk, scratch = setting
                rep = torch.zeros(_lib.DWX_REPLICAS * 3 * C4, device=dev) if scratch else None
                with seg_chunk(chunk):
                    rc = lib.pn2_group_affine_bwd_seg(*common, mem.data_ptr(), own.data_ptr(), B, N, S, K, C, Gm.data_ptr(), ldg,
                                                      dW.data_ptr() + 4 * Dw, Dw + 3, rep.data_ptr() if scratch else None, None, st)
            tag = (name, kind, C, setting)
            assert rc == 0, tag
            Gs.append((tag, Gm.view(B, N, ldg)))
            dWs.append((tag, dW))
        body = [(tag, Gv[:, :, :C]) for tag, Gv in Gs]
        if kind == "exact":
            check_exacts(body, Gref, A, R.EXACT_AFFINE_UNIT_G)
        else:
            check_sums(body, Gref, n, A)
        pad = torch.stack([Gv[:, :, C:] for _, Gv in Gs]).contiguous().view(I32).flatten(1).ne(0).sum(1).cpu()
        for i, (tag, _) in enumerate(Gs):
            assert int(pad[i]) == 0, (tag, "pad columns of G are not zero")
        seen += _check_dwx(kind, dWs, start, Dw, Wref, AW, dY32, rel32)
    return seen


def _report(tag, seen):
    if seen:
        print("%s: dWx kernel %.2e .. %.2e, yardstick %.2e .. %.2e of max|ref|" % (tag, min(e for e, _ in seen), max(e for e, _ in seen),
                                                                                  min(y for _, y in seen), max(y for _, y in seen)))


@pytest.mark.parametrize("C", [4, 6, 16, 32, 48, 50, 64, 96, 128, 256, 1024])
def test_group_affine_bwd_constructed(dev, C):
    """Both backward kernels of the factorised first layer on the constructed indices (S x K = 39 x 35 = 1365 members per
    cloud, the indices of test_interp_bwd_constructed); C = 1024 runs the atomic kernel only (the segmented one takes C <= 256)."""
    B, S, K = 3, 39, 35
    seen = []
    for name, idx, T in _cases(S * K, 100, B):
        seen += _affine_bwd_case(dev, name, idx, B, T, S, K, C, C, atomic=True)
        if C <= 256 and name in ("len17", "len32", "len63", "three_targets"):
            seen += _affine_bwd_case(dev, name + "_dropped", R.with_dropped(idx, T, C), B, T, S, K, C, C + 1, atomic=False)
    _report("affine_bwd constructed C=%d" % C, seen)


def test_group_affine_bwd_seg_rejects_more_than_256_channels(dev):
    lib, st = lib_st()
    B, N, S, K, C = 1, 8, 2, 4, 260
    z = torch.zeros(B * S * K, C, device=dev)
    blk, xyz, ctr = torch.zeros(4 * C, device=dev), torch.zeros(B, N, 3, device=dev), torch.zeros(B, S, 3, device=dev)
    mem, own = invert(torch.zeros(B, S * K, dtype=torch.int64, device=dev), N)
    Gm, dWx = sentinel((B * N, C), dev), torch.zeros(C, 3, device=dev)
    assert lib.pn2_group_affine_bwd_seg(z.data_ptr(), C, z.data_ptr(), C, blk.data_ptr(), xyz.data_ptr(), ctr.data_ptr(), mem.data_ptr(),
                                        own.data_ptr(), B, N, S, K, C, Gm.data_ptr(), C, dWx.data_ptr(), 3, None, None, st) == PN2_EINVAL
    torch.cuda.synchronize()
    assert bool(is_sent(Gm).all()) and float(dWx.abs().max()) == 0.0


@pytest.mark.parametrize("level", ["msg_sa2_k64", "msg_sa2_k128", "ssg_sa4", "cfg5_sa2"])
def test_group_affine_bwd_real_geometry(dev, level):
    """The ball-query index of KITTI-shaped clouds at the product's level sizes."""
    B, n0, N, S, K, radius, C = {"msg_sa2_k64": (16, 4096, 512, 128, 64, 0.4, 128), "msg_sa2_k128": (16, 4096, 512, 128, 128, 0.8, 128),
                                 "ssg_sa4": (16, 4096, 64, 16, 32, 0.8, 256), "cfg5_sa2": (2, 65536, 8192, 2048, 128, 0.8, 128)}[level]
    xn, xs = _level(B, n0, N, S, 40)
    idx3 = U.query_ball_point(radius, K, xn, xs)
    assert int(idx3.min()) >= 0 and int(idx3.max()) < N          # every centre is a point of the cloud: no empty ball
    _report("affine_bwd " + level, _affine_bwd_case(dev, level, idx3.reshape(B, S * K).cpu(), B, N, S, K, C, 9, atomic=True))


def test_group_affine_bwd_seg_grid_stride_loop(dev):
    """C = 256 (one chunk per wave) and B*S*K = 2^19: 8 192 chunks of 64 members (32 768 of 16) over the capped grid of 1024
    workgroups x 4 waves, so every wave strides over two (eight) chunks."""
    B, N, S, K, C = 2, 8192, 2048, 128, 256
    idx = R.random_index(B, S * K, N, 77)
    _report("affine_bwd grid stride", _affine_bwd_case(dev, "grid_stride", idx, B, N, S, K, C, 13, atomic=False, chunks=(64, 16)))


# ---------------------------------------------------------------------------------------------------- pn2_invert_index

@pytest.mark.parametrize("B,M,T,mode", [(3, 5000, 37, "mixed"), (2, 196608, 1024, "mixed"), (2, 40000, 16384, "mixed"), (2, 30000, 16385, "mixed"),
                                        (2, 30000, 20000, "mixed"), (2, 3000, 1, "mixed"), (3, 1, 5, "mixed"), (3, 1, 20000, "mixed"),
                                        (2, 700, 50, "mixed"), (2, 700, 20000, "mixed"), (2, 5000, 37, "all_dropped"),
                                        (2, 5000, 20000, "all_dropped"), (2, 5000, 37, "one_target"), (2, 5000, 20000, "one_target")])
def test_invert_index_members_and_owners(dev, B, M, T, mode):
    """Both implementations (T <= 16 384: one LDS pass; above: three passes) keep the header's contract for members AND
    owners: valid positions grouped by ascending target, each exactly once, and the slots of dropped entries, at the end of
    the cloud's arrays, hold -1 in both."""
    rng = np.random.default_rng(B * M + T)
    idx = rng.integers(0, T, (B, M))
    if mode == "all_dropped":
        idx[:] = np.where(rng.integers(0, 2, (B, M)) == 0, -1, T + 5)
    elif mode == "one_target":
        idx[:] = (np.arange(B) * 7 % T)[:, None]
    if mode != "all_dropped" and M > 1:
        idx[0, ::97] = T + 5
        idx[1, 5::131] = -1
    members, owners = invert(torch.from_numpy(idx).to(dev), T)
    members, owners = members.cpu().numpy(), owners.cpu().numpy()
    for b in range(B):
        valid = (idx[b] >= 0) & (idx[b] < T)
        n = int(valid.sum())
        assert (members[b, n:] == -1).all(), "members: slots of dropped entries"
        assert (owners[b, n:] == -1).all(), "owners: slots of dropped entries"
        mem, own = members[b, :n], owners[b, :n]
        assert (np.diff(own) >= 0).all()
        assert (idx[b][mem] == own).all()
        assert np.array_equal(np.sort(mem), np.nonzero(valid)[0])
