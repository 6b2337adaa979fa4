"""GPU: the conv1x1 entry points at their row thresholds and ragged tails, kernel-level through the C ABI on the fixed
operands of tests/mlp_ref.py, against fp64.

pn2_conv1x1_fwd, pn2_conv1x1_dgrad and pn2_conv1x1_bwd run a leading block of whole tiles in a fast family (weight-resident
fwd_res_kernel / bwd_res_kernel / split_bwd_res_kernel, register-stationary split_nt_kernel / regw_nt_kernel) and hand the
ragged remainder to the streamed kernels on offset pointers; the wide weight gradients pick an instantiation by P % 32 and
P % 16.  Which kernel runs depends on row thresholds that are library options: every case here sits at one of them
(threshold - 1, threshold, threshold + a ragged tail), read from _lib.options().

Every seam case runs the whole-tile part ALONE first -- asserting through pn2_last_kernel() that the family the case is
about was launched, and holding that part to fp64 at its own scale -- and then the ragged call, whose last launch must be
a streamed kernel.  Rows behind the last whole tile are scaled by 32 (mlp_ref: SEAM-SENSITIVE INPUTS), so a tail row that is
dropped or counted twice moves sum y^2, dW and the reductions by far more than the bounds; every output sits in guard rows
and columns (mlp_ref: GUARDS).  Y / dX are held to their bound over the whole-tile rows and over the tail rows separately,
each against that part's own largest entry.

Bounds (none of them fitted to these kernels' results): Y within 2e-6 max|ref| max(1, sqrt(K) / 8) and dx / dW / db by the
same formula with C_out / P / P under the root -- what test_plain_conv1x1_bias_and_weight_gradients holds the streamed
kernels to; sum y and sum y^2 within 1e-5 of sum |y| and sum y^2 -- the rtol of _check_shared_mlp's running statistics;
dX, dW and the two reductions of the BatchNorm layers within 3e-6 of each tensor's largest entry -- the bound of the
fixed-operand tests of tests/test_mlp_gpu.py, on the same operand generator and the same range of row counts.
"""
import ctypes
import itertools
import re

import pytest
import torch

from pointnet12_amd import _lib

import mlp_ref as R

pytestmark = pytest.mark.gpu

STREAMED = ("gemm_nt_kernel", "fewrow_nt_kernel", "gemm_tn_kernel", "wgrad_skinny_kernel")
EPS, MOMENTUM = 1e-5, 0.1


def _thr(base):
    o = _lib.options()
    return {"R": o["PN2_RES_MIN_ROWS"], "Wd": o["PN2_WIDE_MIN_ROWS"], "S128": o["PN2_SPLIT_MIN_ROWS_128"],
            "G": o["PN2_WIDE_WGRAD_MIN_ROWS"], "T128": 64 * o["PN2_SPLIT_RES_MIN_TILES_128"]}[base]


def _last(lib):
    k = lib.pn2_last_kernel()
    return k.decode() if k else ""


def _is(name, family):
    """`family` is the kernel template `name` instantiates (bwd_res_kernel is not split_bwd_res_kernel)."""
    return re.search(r"(^|[\s:])" + family + r"<", name) is not None


def _streamed(name):
    return any(_is(name, f) for f in STREAMED)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _parts(got, ref, head):
    """Largest error over the rows [0, head) and [head, P), each relative to that part's largest reference entry."""
    return tuple(R.rel(got[lo:hi], ref[lo:hi]) for lo, hi in ((0, head), (head, ref.shape[0])) if hi > lo)


def _stat_sums(stats, C):
    return stats.view(R.STAT_REPLICAS, 2, C).sum(0)


# =============================================================================================== (a) forward

def _fwd(lib, c, Yb, P, K, N, stats, lazy=None):
    rc = lib.pn2_conv1x1_fwd(c["X"].data_ptr(), c["ldx"], _p(c["aff"]), c["W"].data_ptr(), c["ldw"], c["bias"].data_ptr(), Yb.data_ptr(),
                             c["ldy"], P, K, N, _p(stats), lazy, _stream())
    assert rc == 0, rc
    return _last(lib)


def _check_fwd(dev, Yb, stats, ref, lo, hi, K, N, what):
    """Y rows [lo, hi) and the sums over them against fp64; returns the measured (Y, sum y, sum y^2) errors in units of
    their bounds' scales."""
    torch.cuda.synchronize()
    R.check_guards(Yb, hi - lo, N, what)
    Yr = ref["Y"][lo:hi]
    e_y = R.rel(Yb[:hi - lo, :N], Yr)
    s = _stat_sums(stats, N)
    e_s1 = float(((s[0] - Yr.sum(0)).abs() / Yr.abs().sum(0)).max())
    e_s2 = float(((s[1] - (Yr * Yr).sum(0)).abs() / (Yr * Yr).sum(0)).max())
    return e_y, e_s1, e_s2


def _y_tol(K):
    return 2e-6 * max(1.0, K ** 0.5 / 8)


def _fwd_seam_case(dev, family, tile, K, N, P, thr, affine, seed):
    """One row of the tables of (a).  family None: no fast family takes the shape at all (the whole call is streamed)."""
    lib = _lib.load()
    head = (P // tile) * tile if (family and P >= thr) else 0
    c, ref = R.fixed_forward_case(dev, P, K, N, seed, affine=affine, ldy=R.round4(N) + (0 if affine else 8),
                                  tail_from=head if 0 < head < P else None)
    tol = _y_tol(K)
    if 0 < head < P:                                                # the whole-tile part alone: the family this case is about
        Yh, st_h = R.guarded(head, c["ldy"], dev), torch.zeros(R.STAT_REPLICAS * 2 * N, device=dev, dtype=torch.float64)
        name = _fwd(lib, c, Yh, head, K, N, st_h)
        assert _is(name, family), (family, name)
        e = _check_fwd(dev, Yh, st_h, ref, 0, head, K, N, "Y of the whole tiles alone")
        print("fwd %s %d -> %d, %d rows alone (affine %d): Y %.2e  sums %.2e %.2e" % ((family, K, N, head, affine) + e))
        assert e[0] <= tol and e[1] <= 1e-5 and e[2] <= 1e-5, e
    Yb, stats = R.guarded(P, c["ldy"], dev), torch.zeros(R.STAT_REPLICAS * 2 * N, device=dev, dtype=torch.float64)
    name = _fwd(lib, c, Yb, P, K, N, stats)
    _, e_s1, e_s2 = _check_fwd(dev, Yb, stats, ref, 0, P, K, N, "Y")
    e_y = _parts(Yb[:P, :N], ref["Y"], head)
    print("fwd %s %d -> %d, P = %d = %d + %d (affine %d): Y %s  sums %.2e %.2e  [%s]" %
          (family, K, N, P, head, P - head, affine, " ".join("%.2e" % v for v in e_y), e_s1, e_s2, name[:60]))
    assert max(e_y) <= tol and e_s1 <= 1e-5 and e_s2 <= 1e-5, (e_y, e_s1, e_s2)
    if head == P:
        assert _is(name, family), (family, name)
    else:
        assert _streamed(name), name                                # the tail's launch (threshold - 1: the only launch)


def _fwd_params():
    out = []
    for K, N in ((32, 32), (64, 64), (96, 128), (128, 32)):
        out += [("fwd_res_kernel", 32, K, N, "R", d) for d in (-1, 0, 1, 31, 33)]
    # W [128, 132] plus eight staging buffers do not fit the LDS: 128 -> 64 / 96 / 128 have no weight-resident forward
    # (launch_fwd_res), the streamed kernel takes all rows on either side of the threshold
    out += [(None, 32, 128, 64, "R", d) for d in (-1, 0, 1, 31, 33)]
    out += [(None, 32, 128, 128, "S128", -1)]
    for K, N in ((128, 256), (128, 196), (196, 256)):
        out += [("split_nt_kernel", 64, K, N, "Wd", d) for d in (0, 1, 63, 65)]
    out += [("split_nt_kernel", 64, 128, 128, "S128", d) for d in (0, 63)]
    out += [("split_nt_kernel", 128, 64, 96, "Wd", d) for d in (1, 127)]
    return [pytest.param(*p, a, id="%s-%dx%d-%s%+d-%s" % (p[0] or "streamed", p[2], p[3], p[4], p[5], "bn" if a else "plain"))
            for p in out for a in (True, False)]


@pytest.mark.parametrize("family,tile,K,N,base,delta,affine", _fwd_params())
def test_forward_at_the_row_thresholds_and_ragged_tails(dev, family, tile, K, N, base, delta, affine):
    """(a) pn2_conv1x1_fwd with stats, with and without an input BatchNorm block, around RES_MIN_ROWS (fwd_res_kernel, 32-row
    slabs), WIDE_MIN_ROWS and SPLIT_MIN_ROWS_128 (split_nt_kernel, 64-row tiles; 128 for 64 -> 96).  128 -> 64 and 128 -> 128
    below SPLIT_MIN_ROWS_128 have no resident kernel (LDS): asserted to run streamed as a whole; 128 -> 32 stands in as the
    resident K = 128 form."""
    thr = _thr(base)
    if family == "split_nt_kernel" and K == 64:
        assert _lib.options()["PN2_SPLIT_NARROW"] == 1
    _fwd_seam_case(dev, family, tile, K, N, thr + delta, thr, affine, 1000 + K + N + delta)


@pytest.mark.parametrize("K,N", [(128, 256), (196, 256)])
def test_forward_of_the_fp32_register_stationary_kernel_with_a_ragged_tail(dev, K, N):
    """(a) regw_nt_kernel (PN2_SPLIT=0: the fp32 form of the wide forward, 128-row tiles) at WIDE_MIN_ROWS + 127."""
    old = _lib.options()["PN2_SPLIT"]
    _lib.set_option("PN2_SPLIT", 0)
    try:
        thr = _thr("Wd")
        for affine in (True, False):
            _fwd_seam_case(dev, "regw_nt_kernel", 128, K, N, thr + 127, thr, affine, 2000 + K + N)
    finally:
        _lib.set_option("PN2_SPLIT", old)


# =============================================================================================== (b), (c) backward

def _bwd_outputs(dev, c, P, co, ci, seed, wide):
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    ldxo = c["ldp"] + (8 if wide else 0)
    dW, dW0 = R.framed(co, ci, ci + 4, rnd)
    return dict(dX=R.guarded(P, ldxo, dev), ldxo=ldxo, dW=dW, dW0=dW0, lddw=ci + 4,
                red=torch.zeros(R.STAT_REPLICAS * 2 * ci, device=dev, dtype=torch.float64) if c["affp"] is not None else None)


def _dgrad(lib, c, o, P, co, ci, lazy=None):
    rc = lib.pn2_conv1x1_dgrad(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), c["ldw"],
                               c["Yp"].data_ptr() if c["affp"] is not None else None, c["ldp"], _p(c["affp"]), o["dX"].data_ptr(), o["ldxo"],
                               _p(o["red"]), P, co, ci, lazy, _stream())
    assert rc == 0, rc
    return _last(lib)


def _wgrad(lib, c, o, P, co, ci, lazy=None, dbias=None):
    rc = lib.pn2_conv1x1_wgrad(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["Yp"].data_ptr(), c["ldp"], _p(c["affp"]),
                               o["dW"].data_ptr(), o["lddw"], _p(dbias), P, co, ci, lazy, _stream())
    assert rc == 0, rc
    return _last(lib)


def _bwd(lib, c, o, P, co, ci, lazy=None):
    rc = lib.pn2_conv1x1_bwd(*c["dz_args"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), c["ldw"], c["Yp"].data_ptr(),
                             c["ldp"], _p(c["affp"]), o["dX"].data_ptr(), o["ldxo"], _p(o["red"]), o["dW"].data_ptr(), o["lddw"], P, co, ci,
                             lazy, _stream())
    assert rc == 0, rc
    return _last(lib)


def _check_bwd(o, ref, rows, co, ci, head, what, dW=True):
    """The outputs of a backward over the rows [0, rows) against fp64: (dX errors per part, dW, red0, red1) in units of each
    tensor's largest entry; guard rows / columns of dX and the frame of dW untouched."""
    torch.cuda.synchronize()
    sums = ref["part"](0, rows)
    R.check_guards(o["dX"], rows, ci, "dX " + what)
    R.check_frame(o["dW"], o["dW0"], co, ci, "dW " + what)
    errs = list(_parts(o["dX"][:rows, :ci], ref["dX"][:rows], head))
    if dW:
        errs.append(R.rel(o["dW"][:co, :ci], o["dW0"][:co, :ci].double() + sums["dW"]))
    if o["red"] is not None:
        red = _stat_sums(o["red"], ci)
        errs += [R.rel(red[0], sums["r0"]), R.rel(red[1], sums["r1"])]
    return tuple(errs)


def _fmt(errs):
    return " ".join("%.2e" % e for e in errs)


WGRAD_KERNEL = {"streamed": r"gemm_tn_kernel<", "split16": r"split_tn_kernel<[^>]*, 16>", "split32": r"split_tn_kernel<[^>]*, 32>",
                "full": r"wgrad_full_kernel<"}


@pytest.mark.parametrize("co,ci,Kp,base,delta,wg", [
    (196, 128, 0, "Wd", 1, "streamed"), (196, 128, 0, "Wd", 63, "streamed"), (128, 128, 0, "S128", 33, "streamed"),
    (196, 128, 0, "G", -1, "streamed"), (196, 128, 0, "G", 16, "split16"), (196, 128, 0, "G", 8, "full"), (196, 128, 0, "G", 1, "full"),
    (256, 128, 64, "G", 64, "split32"), (256, 196, 128, "G", 128, "split16")])
def test_wide_dgrad_and_wgrad_at_the_row_thresholds_and_ragged_tails(dev, co, ci, Kp, base, delta, wg):
    """(b) pn2_conv1x1_dgrad + pn2_conv1x1_wgrad of the wide layers.  Dense: split_nt_kernel takes whole 64-row tiles and the
    streamed kernel the rest; the weight gradient is streamed below WIDE_WGRAD_MIN_ROWS, split_tn_kernel with 16-row chunks
    where P % 32 != 0 = P % 16, and the fp32 wgrad_full_kernel with a ragged last chunk where P % 16 != 0.  Pooled (whole
    groups, so no streamed tail): P / 256 workgroups' shares that are no whole number of groups -- the rows_per_wg rounding
    of launch_split_tn -- in split_nt_kernel and split_tn_kernel (32-row chunks at 256 x 128, 16-row at 256 x 196: the pooled
    BP = 16 forms of 256 x 128 need P % 32 != 0, which no multiple of Kpool = 64 / 128 is -- unreachable)."""
    lib = _lib.load()
    P = _thr(base) + delta
    head = P if Kp else (P // 64) * 64
    c, ref = R.fixed_layer_case(dev, P, co, ci, Kp, 3000 + co + ci + Kp + delta, tail_from=head if head < P else None)
    if head < P:                                                    # the whole tiles alone
        o = _bwd_outputs(dev, c, head, co, ci, 5, wide=True)
        name = _dgrad(lib, c, o, head, co, ci)
        assert _is(name, "split_nt_kernel"), name
        e = _check_bwd(o, ref, head, co, ci, head, "of the whole tiles alone", dW=False)
        print("dgrad %d x %d, %d rows alone: dX, red %s" % (co, ci, head, _fmt(e)))
        assert max(e) <= 3e-6, e
    o = _bwd_outputs(dev, c, P, co, ci, 6, wide=True)
    name_d = _dgrad(lib, c, o, P, co, ci)
    assert _streamed(name_d) if head < P else _is(name_d, "split_nt_kernel"), name_d
    name_w = _wgrad(lib, c, o, P, co, ci)
    assert re.search(WGRAD_KERNEL[wg], name_w), (wg, name_w)
    e = _check_bwd(o, ref, P, co, ci, head, "")
    print("dgrad + wgrad %d x %d, K=%d, P = %d = %d + %d: dX%s, dW, red %s  [%s | %s]" %
          (co, ci, Kp, P, head, P - head, " (head, tail)" if head < P else "", _fmt(e), name_d[:48], name_w[:56]))
    assert max(e) <= 3e-6, e


@pytest.mark.parametrize("co,ci,Kp,masked,family,base,delta", [
    (32, 32, 0, True, "bwd_res_kernel", "R", 1), (32, 32, 0, True, "bwd_res_kernel", "R", 31), (32, 32, 0, True, "bwd_res_kernel", "R", 63),
    (64, 64, 0, True, "split_bwd_res_kernel", "R", 1), (64, 64, 0, True, "split_bwd_res_kernel", "R", 31),
    (64, 64, 0, True, "split_bwd_res_kernel", "R", 63),
    (96, 64, 0, True, "split_bwd_res_kernel", "R", 1), (96, 64, 0, True, "split_bwd_res_kernel", "R", 31),
    (96, 64, 0, True, "split_bwd_res_kernel", "R", 63),
    (128, 128, 0, True, "split_bwd_res_kernel", "T128", -1), (128, 128, 0, True, "split_bwd_res_kernel", "T128", 1),
    (128, 128, 0, True, "split_bwd_res_kernel", "T128", 63), (128, 128, 0, False, "split_bwd_res_kernel", "T128", 63),
    (64, 32, 32, True, "bwd_res_kernel", "R", 32), (128, 64, 32, True, "split_bwd_res_kernel", "R", 32)])
def test_fused_backward_with_a_ragged_tail(dev, co, ci, Kp, masked, family, base, delta):
    """(c) pn2_conv1x1_bwd: whole 64-row tiles in the fused kernel, the rest through pn2_conv1x1_dgrad + pn2_conv1x1_wgrad on
    offset pointers, dW and the reductions accumulated over both.  128 x 128 below SPLIT_RES_MIN_TILES_128 tiles runs
    streamed as a whole; the unmasked form (no previous BatchNorm: prev_affine = prev_red = NULL); pooled over 32 with one
    whole group behind the last tile (the dZp / arg offset of the tail)."""
    lib = _lib.load()
    thr = _thr(base)
    P = thr + delta
    head = (P // 64) * 64 if P >= thr else 0
    c, ref = R.fixed_layer_case(dev, P, co, ci, Kp, 4000 + co + ci + Kp + delta, masked=masked, tail_from=head if head else None)
    if head:
        o = _bwd_outputs(dev, c, head, co, ci, 7, wide=True)
        name = _bwd(lib, c, o, head, co, ci)
        assert _is(name, family), (family, name)
        e = _check_bwd(o, ref, head, co, ci, head, "of the whole tiles alone")
        print("bwd %d x %d, K=%d, %d rows alone: dX, dW, red %s" % (co, ci, Kp, head, _fmt(e)))
        assert max(e) <= 3e-6, e
    o = _bwd_outputs(dev, c, P, co, ci, 8, wide=True)
    name = _bwd(lib, c, o, P, co, ci)
    assert _streamed(name), name
    e = _check_bwd(o, ref, P, co, ci, head, "")
    print("bwd %d x %d, K=%d, masked %d, P = %d = %d + %d: dX%s, dW, red %s  [%s]" %
          (co, ci, Kp, masked, P, head, P - head, " (head, tail)" if head else "", _fmt(e), name[:56]))
    assert max(e) <= 3e-6, e


# =============================================================================================== (d) lazy blocks across a seam

def _block_err(got, ref):
    """Largest error of a [4, C] block, each row relative to its own largest entry."""
    return max(R.rel(got[i], ref[i]) for i in range(4))


@pytest.mark.parametrize("K,N,base,delta", [(64, 64, "R", 17), (128, 256, "Wd", 65)])
def test_lazy_affine_block_across_a_forward_seam(dev, K, N, base, delta):
    """(d) pn2_conv1x1_fwd with in_lazy on a ragged row count: the head launch realises the input's BatchNorm block and
    updates the running statistics, the tail launch must read the block and update nothing.  Against the same call on a
    block written beforehand by pn2_bn_finalize: block, Y, running statistics bit-equal, num_batches_tracked == 1, the sums
    within the bounds of (a) (their atomics land in another order), the block within 1e-6 of fp64."""
    lib = _lib.load()
    P = _thr(base) + delta
    tile = 32 if base == "R" else 64
    head = (P // tile) * tile
    c, _ = R.fixed_forward_case(dev, P, K, N, 5000 + K + N, affine=False, tail_from=head)
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    gamma, beta = rnd(K) * 0.5 + 1.0, rnd(K) * 0.3
    gamma[::7] *= -1.0
    xd = c["X"][:, :K].double()
    s1, s2 = xd.sum(0), (xd * xd).sum(0)
    stats_in = R.replicate(torch.stack([s1, s2]))
    rm0, rv0 = rnd(K) * 0.1, rnd(K).abs() + 0.5
    runs = []
    for lazy_run in (False, True):
        aff = torch.zeros(4 * K, device=dev)
        rm, rv, nbt = rm0.clone(), rv0.clone(), torch.zeros(1, device=dev, dtype=torch.int64)
        Yb, stats = R.guarded(P, c["ldy"], dev), torch.zeros(R.STAT_REPLICAS * 2 * N, device=dev, dtype=torch.float64)
        cc = dict(c, aff=aff)
        if lazy_run:
            z = _lib.BnLazy(stats_in.data_ptr(), gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(),
                            aff.data_ptr(), P, K)
            name = _fwd(lib, cc, Yb, P, K, N, stats, ctypes.byref(z))
        else:
            assert lib.pn2_bn_finalize(stats_in.data_ptr(), P, K, gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, 1, rm.data_ptr(), rv.data_ptr(),
                                       nbt.data_ptr(), aff.data_ptr(), _stream()) == 0
            name = _fwd(lib, cc, Yb, P, K, N, stats)
        assert _streamed(name), name
        torch.cuda.synchronize()
        R.check_guards(Yb, P, N, "Y")
        runs.append((aff, Yb, rm, rv, nbt, stats))
    (aff1, Y1, rm1, rv1, nbt1, st1), (aff2, Y2, rm2, rv2, nbt2, st2) = runs
    assert torch.equal(aff1, aff2) and torch.equal(Y1[:P], Y2[:P])
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and int(nbt1) == 1 and int(nbt2) == 1
    blk = R.affine_block(s1, s2, P, gamma, beta, EPS)
    rm_ref, rv_ref = R.running_stats(s1, s2, P, MOMENTUM, rm0, rv0)
    e_blk, e_rm, e_rv = _block_err(aff2.view(4, K), blk), R.rel(rm2, rm_ref), R.rel(rv2, rv_ref)
    act = R.bn_relu(c["X"][:, :K], aff2.view(4, K))[0]
    Yr = act @ c["W"].double().t() + c["bias"].double()
    e_y = _parts(Y2[:P, :N], Yr, head)
    e_s = []
    for st in (st1, st2):
        s = _stat_sums(st, N)
        e_s += [float(((s[0] - Yr.sum(0)).abs() / Yr.abs().sum(0)).max()), float(((s[1] - (Yr * Yr).sum(0)).abs() / (Yr * Yr).sum(0)).max())]
    print("lazy fwd %d -> %d, P = %d: block %.2e  running %.2e %.2e  Y %s  sums %s" % (K, N, P, e_blk, e_rm, e_rv, _fmt(e_y), _fmt(e_s)))
    assert e_blk <= 1e-6 and e_rm <= 1e-6 and e_rv <= 1e-6
    assert max(e_y) <= _y_tol(K) and max(e_s) <= 1e-5


@pytest.mark.parametrize("kind,co,ci,base,delta", [("bwd", 96, 64, "R", 31), ("dgrad", 196, 128, "Wd", 1), ("wgrad", 196, 128, "G", 8)])
def test_lazy_coefficient_block_across_a_backward_seam(dev, kind, co, ci, base, delta):
    """(d) pn2_conv1x1_bwd / _dgrad / _wgrad with coef_lazy on a ragged row count, against the same call on a block written
    beforehand by pn2_bn_bwd_coef: block and dX bit-equal, dgamma / dbeta (accumulate = 1) bit-equal and added to exactly
    once, dW and the reductions within the bounds of (b) / (c), the block within 1e-6 of fp64."""
    lib = _lib.load()
    P = _thr(base) + delta
    head = (P // 64) * 64 if kind != "wgrad" else P
    g = torch.Generator(device=dev).manual_seed(6)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    c4 = R.round4(co)
    aff_l = R.draw_affine(rnd, co, c4, dev)                        # this layer's own affine block
    gamma = rnd(co) * 0.5 + 1.0
    gamma[::5] *= -1.0
    r01 = torch.randn(2, co, device=dev, dtype=torch.float64, generator=g) * P ** 0.5
    red_in = R.replicate(r01)
    dg0, db0 = rnd(co), rnd(co)
    runs = []
    for lazy_run in (False, True):
        coef = torch.zeros(4 * c4, device=dev)
        dg, db = dg0.clone(), db0.clone()
        if lazy_run:
            z = _lib.BnCoefLazy(red_in.data_ptr(), gamma.data_ptr(), aff_l.data_ptr(), coef.data_ptr(), dg.data_ptr(), db.data_ptr(), 1, P, co)
            lazy = ctypes.byref(z)
        else:
            assert lib.pn2_bn_bwd_coef(red_in.data_ptr(), P, co, gamma.data_ptr(), aff_l.data_ptr(), 1, coef.data_ptr(), dg.data_ptr(),
                                       db.data_ptr(), 1, _stream()) == 0
            lazy = None
        c, ref = R.fixed_layer_case(dev, P, co, ci, 0, 6000 + co + ci, tail_from=head if head < P else None, coef=coef)
        o = _bwd_outputs(dev, c, P, co, ci, 9, wide=False)
        if kind == "bwd":
            name = _bwd(lib, c, o, P, co, ci, lazy)
        elif kind == "dgrad":
            name = _dgrad(lib, c, o, P, co, ci, lazy)
        else:
            name = _wgrad(lib, c, o, P, co, ci, lazy)
        assert _is(name, "wgrad_full_kernel") if kind == "wgrad" else _streamed(name), name
        torch.cuda.synchronize()
        runs.append((coef, dg, db, o, ref))
    (coef1, dg1, db1, o1, ref), (coef2, dg2, db2, o2, _) = runs       # (the statement of the run whose block existed when it was made)
    assert torch.equal(coef1, coef2)
    assert torch.equal(dg1, dg2) and torch.equal(db1, db2)
    assert torch.equal(dg2, dg0 + r01[1].float()) and torch.equal(db2, db0 + r01[0].float())      # added to exactly once
    a = aff_l.view(4, c4)[:, :co]
    e_blk = _block_err(coef2.view(4, c4)[:, :co], R.coef_block(r01[0], r01[1], P, gamma, a[0], a[3]))
    errs = []
    for o in (o1, o2):
        if kind == "wgrad":
            R.check_frame(o["dW"], o["dW0"], co, ci, "dW")
            errs.append(R.rel(o["dW"][:co, :ci], o["dW0"][:co, :ci].double() + ref["dW"]))
        else:
            errs += list(_check_bwd(o, ref, P, co, ci, head, "", dW=kind == "bwd"))
    if kind != "wgrad":
        assert torch.equal(o1["dX"][:P], o2["dX"][:P])
    print("lazy %s %d x %d, P = %d: block %.2e  outputs (both runs) %s" % (kind, co, ci, P, e_blk, _fmt(errs)))
    assert e_blk <= 1e-6 and max(errs) <= 3e-6, (e_blk, errs)


# =============================================================================================== (e) streamed kernels, small and odd

def _small_params():
    Ps, Ks, Ns = (1, 31, 33, 65, 130), (1, 3, 9, 137), (1, 13, 33, 129, 196, 224, 225)
    out = []
    for i, (P, K) in enumerate(itertools.product(Ps, Ks)):          # every (P, K) with two of the N, both weight layouts in turn
        for j, n in enumerate((Ns[i % 7], Ns[(3 * i + 2) % 7])):
            out.append((P, K, n, ("slice", "padded")[(i + j) % 2]))
    return out


@pytest.mark.parametrize("P,K,N,w_mode", _small_params())
def test_streamed_kernels_on_small_and_odd_shapes(dev, P, K, N, w_mode):
    """(e) pn2_conv1x1_fwd, pn2_conv1x1_dgrad (first layer: prev_Y = NULL) and pn2_conv1x1_wgrad (with and without dbias) of one
    layer K -> N on P rows in the streamed kernels: row counts around the 32- and 64-row tiles, contraction lengths that are
    no multiple of 4, output widths across the narrow tiles (33, 129) and the 128 + remainder rule (224, 225), pitches
    round4(K) + 4 and round4(N) + 8 with large values in the extra columns, W as columns [3, 3 + K) of an [N, K + 3] matrix
    (guarded scalar loads) or as a 16-byte aligned zero-padded copy (float4 loads).  Bounds: the formula of
    test_plain_conv1x1_bias_and_weight_gradients."""
    lib = _lib.load()
    ldk, ldn = R.round4(K) + 4, R.round4(N) + 8
    seed = 7000 + 131 * P + 7 * K + N
    cf, rf = R.fixed_forward_case(dev, P, K, N, seed, affine=False, ldx=ldk, ldy=ldn, w_mode=w_mode)
    Yb, stats = R.guarded(P, ldn, dev), torch.zeros(R.STAT_REPLICAS * 2 * N, device=dev, dtype=torch.float64)
    names = [_fwd(lib, cf, Yb, P, K, N, stats)]
    _check_fwd(dev, Yb, stats, rf, 0, P, K, N, "Y")
    # the sums of a handful of rows cannot be better than Y itself: with every y within d = the bound of Y, sum y is within
    # P d and sum y^2 within 2 d sum |y| + P d^2 (a relative bound like (a)'s has no meaning for a y that cancels to ~0 in a
    # sum of one row); a dropped row would move them by ~|y| and ~y^2
    d = _y_tol(K) * float(rf["Y"].abs().max())
    s = _stat_sums(stats, N)
    e_s1 = float((s[0] - rf["s1"]).abs().max()) / (P * d)
    e_s2 = float(((s[1] - rf["s2"]).abs() / (2 * d * rf["sabs"] + P * d * d)).max())

    c, ref = R.fixed_layer_case(dev, P, N, K, 0, seed + 1, masked=False, ldc=ldn, ldp=ldk, w_mode=w_mode)
    o = _bwd_outputs(dev, c, P, N, K, 10, wide=False)
    names.append(_dgrad(lib, c, o, P, N, K))
    names.append(_wgrad(lib, c, o, P, N, K))
    torch.cuda.synchronize()
    R.check_guards(o["dX"], P, K, "dx")
    R.check_frame(o["dW"], o["dW0"], N, K, "dW")
    g = torch.Generator(device=dev).manual_seed(11)
    o2 = dict(o, dW=o["dW0"].clone())
    dbias, dbias0 = R.framed(1, N, N + 4, lambda *s_: torch.randn(*s_, device=dev, generator=g))
    names.append(_wgrad(lib, c, o2, P, N, K, dbias=dbias))
    torch.cuda.synchronize()
    R.check_frame(o2["dW"], o["dW0"], N, K, "dW (with dbias)")
    R.check_frame(dbias, dbias0, 1, N, "dbias")
    assert all(_streamed(n) for n in names), names

    def err(got, want, n):                                         # in units of the bound
        return float((got.double() - want).abs().max()) / (2e-6 * max(float(want.abs().max()), 1e-30) * max(1.0, n ** 0.5 / 8))
    dW_ref = o["dW0"][:N, :K].double() + ref["dW"]
    errs = (err(Yb[:P, :N], rf["Y"], K), err(o["dX"][:P, :K], ref["dX"], N), err(o["dW"][:N, :K], dW_ref, P), err(o2["dW"][:N, :K], dW_ref, P),
            err(dbias[0, :N], dbias0[0, :N].double() + ref["db"], P))
    errs += (e_s1, e_s2)
    print("small %d x %d -> %d (%s): y, dx, dW, dW (with dbias), db, sum y, sum y^2 in units of their bounds %s" %
          (P, K, N, w_mode, " ".join("%.3f" % e for e in errs)))
    assert max(errs) <= 1.0, errs
