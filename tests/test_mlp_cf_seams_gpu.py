"""GPU: the closed-form / output-free conv1x1 entry points the default training step runs -- pn2_conv1x1_bwd_cf
(split_bwd_cf_kernel with cf_prep_kernel / cf_finish_kernel), pn2_conv1x1_bwd_first (split_bwd_res_kernel, FUSE0) with its
finishing pn2_conv1x1_wgrad_cf(dZ = NULL), and pn2_conv1x1_wgrad_cf with dZ (wgrad_first_cf_kernel) -- kernel-level through the
C ABI on the fixed operands of tests/mlp_cf_ref.py, against fp64, at their seams: the row threshold (read from
_lib.options()) and the trip counts around the grid cap (read from the device), every group size, every arg pattern, pitches
beyond the width with NaN behind it, the lazy coefficient record, a coefficient block with the cancellation of a real BatchNorm
backward, N0 below 12, and -- with PN2_RES_MIN_ROWS lowered for the test -- one to 2 g + 1 chunks, which drives
cf_finish_kernel's two slab loops through every remainder, the prefetch past the last chunk, one-trip workgroups and
chunks == grid.  After every call pn2_last_kernel() must name the kernel the case is about.

Every output sits in guard rows / a frame (mlp_ref: GUARDS), pn2_conv1x1_bwd_cf's scratch is NaN-filled (its contract: contents
need not be initialised), both scratch buffers end in guard words.

Bounds, none fitted to a GPU result (mlp_cf_ref: BOUNDS): dX, dW, dW0 and the two reductions within 3e-6 of the reference
tensor's largest entry, dX over scaled rows and the rest separately; in the cases whose largest entry is a cancelled sum (the
self-consistent and large-q1 blocks) max(3e-6, 4 e32) with e32 the error of the textbook form in plain float32 torch arithmetic.
tests/test_mlp_cf_ref_cpu.py shows a float32 emulation of the kernels' closed forms inside these bounds and ten mutants outside.
"""
import ctypes
import re

import pytest
import torch

from pointnet12_amd import _lib

import mlp_cf_ref as C
import mlp_ref as R
import options_ref as O

pytestmark = pytest.mark.gpu

SHAPES_CF, SHAPES_FIRST = ((128, 96), (128, 64)), ((96, 64), (64, 64))
GUARD_BYTES = 256


@pytest.fixture(autouse=True)
def _routes_under_test(dev):
    """FUSE_FIRST = 1 and POOL_CF = 2 (the defaults) for every test of this file, set so that the file says what it tests."""
    with O.options(PN2_FUSE_FIRST=1, PN2_POOL_CF=2):
        yield


def _thr():
    return _lib.options()["PN2_RES_MIN_ROWS"]


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _last(lib):
    k = lib.pn2_last_kernel()
    return k.decode() if k else ""


def _is(name, pattern):
    return re.search(r"(^|[\s:])" + pattern, name) is not None


FUSE0_KERNEL = r"split_bwd_res_kernel<\s*\d+,\s*\d+,\s*false,\s*true,\s*true\s*>"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rnd(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return lambda *s_: torch.randn(*s_, device=dev, generator=g)


def _scratch(nbytes, dev, fill):
    """`nbytes` of scratch filled with the byte `fill` in front of GUARD_BYTES guard bytes (0xA5)."""
    buf = torch.full((nbytes + GUARD_BYTES,), fill, device=dev, dtype=torch.uint8)
    buf[nbytes:] = 0xA5
    assert buf.data_ptr() % 256 == 0
    return buf


def _scratch_intact(buf, what):
    assert bool((buf[-GUARD_BYTES:] == 0xA5).all()), "%s: written past its end" % what


def _fmt(errs):
    return " ".join("%.2e" % e for e in errs)


def _stat_sums(red, C_):
    return red.view(R.STAT_REPLICAS, 2, C_).sum(0)


# =============================================================================================== pn2_conv1x1_bwd_cf

def _cf_outputs(dev, P, co, ci, pitches, seed=1):
    ldxo, lddw = pitches.get("ldxo", ci), pitches.get("lddw", ci)
    dW, dW0 = R.framed(co, ci, lddw, _rnd(dev, seed))
    nbytes = int(_lib.load().pn2_conv1x1_bwd_cf_scratch_bytes(co, ci))
    return dict(dX=R.guarded(P, ldxo, dev), ldxo=ldxo, dW=dW, dW0=dW0, lddw=lddw, scratch=_scratch(nbytes, dev, 0xFF),     # (0xFFFFFFFF: a NaN)
                red=torch.zeros(R.STAT_REPLICAS * 2 * ci, device=dev, dtype=torch.float64))


def _cf_call(lib, c, o, P, co, ci, lazy=None):
    lib.pn2_clear_last_kernel()
    return lib.pn2_conv1x1_bwd_cf(c["dzp"].data_ptr(), c["ldo"], c["arg"].data_ptr(), c["Kp"], c["coef"].data_ptr(), c["W"].data_ptr(), c["ldw"],
                                  c["bias"].data_ptr(), c["Yp"].data_ptr(), c["ldp"], c["affp"].data_ptr(), o["dX"].data_ptr(), o["ldxo"],
                                  o["red"].data_ptr(), o["dW"].data_ptr(), o["lddw"], P, co, ci, lazy, o["scratch"].data_ptr(), _stream())


def _cf_run(lib, c, o, P, co, ci, lazy=None):
    assert lib.pn2_conv1x1_bwd_cf_supported(P, co, ci, c["Kp"]) == 1
    rc = _cf_call(lib, c, o, P, co, ci, lazy)
    assert rc == 0, rc
    name = _last(lib)
    assert _is(name, r"split_bwd_cf_kernel<\s*4,\s*%d\s*>" % (ci // 32)), name
    torch.cuda.synchronize()


def _cf_untouched(o, ci):
    bits = o["dX"].view(torch.int32)
    return bool((bits == R.SENTINEL).all()) and torch.equal(o["dW"], o["dW0"]) and float(o["red"].abs().max()) == 0.0


def _cf_errors(o, ref, P, co, ci, head=None):
    """(dX per part, dW, red0, red1) of a finished call and the same of the float32 textbook form, each relative to the
    reference's largest entry; guards, frame and the scratch's end checked."""
    R.check_guards(o["dX"], P, ci, "dX")
    R.check_frame(o["dW"], o["dW0"], co, ci, "dW")
    _scratch_intact(o["scratch"], "scratch")
    parts = ((0, P),) if head is None else ((0, head), (head, P))
    dW_ref = o["dW0"][:co, :ci].double() + ref["dW"]
    red = _stat_sums(o["red"], ci)
    f32 = ref["f32"]
    got = [R.rel(o["dX"][lo:hi, :ci], ref["dX"][lo:hi]) for lo, hi in parts] + [R.rel(o["dW"][:co, :ci], dW_ref), R.rel(red[0], ref["r0"]), R.rel(red[1], ref["r1"])]
    e32 = [R.rel(f32["dX"][lo:hi], ref["dX"][lo:hi]) for lo, hi in parts] + [R.rel(o["dW0"][:co, :ci].double() + f32["dW"].double(), dW_ref),
                                                                             R.rel(f32["r0"], ref["r0"]), R.rel(f32["r1"], ref["r1"])]
    return got, [C.bound(ref["kind"], e) for e in e32]


CF_PARAMS = [pytest.param(co, ci, name, id="%dx%d-%s" % (co, ci, name)) for co, ci in SHAPES_CF for name in C.BWD_CF_NAMES]
assert len(CF_PARAMS) == 2 * 21, len(CF_PARAMS)


@pytest.mark.parametrize("co,ci,name", CF_PARAMS)
def test_pooled_backward_from_the_input_at_its_seams(dev, co, ci, name):
    """One row of mlp_cf_ref.bwd_cf_table at R = PN2_RES_MIN_ROWS and g = min(CUs, 256), the grid cap of launch_split_bwd_cf."""
    lib = _lib.load()
    P, Kp, kw, pitches = C.bwd_cf_table(_thr(), min(_cus(dev), 256), co, ci)[name]
    c, ref = C.bwd_cf_case(dev, P, co, ci, Kp, 100 + sum(map(ord, name)) + ci, **kw)
    o = _cf_outputs(dev, P, co, ci, pitches)
    _cf_run(lib, c, o, P, co, ci)
    if kw.get("zero_dzp"):                                          # exactness: nothing in, nothing out, bit for bit
        R.check_guards(o["dX"], P, ci, "dX")
        assert float(o["dX"][:P, :ci].abs().max()) == 0.0 and float(o["red"].abs().max()) == 0.0 and torch.equal(o["dW"], o["dW0"])
        _scratch_intact(o["scratch"], "scratch")
        return
    got, bounds = _cf_errors(o, ref, P, co, ci, kw.get("tail_from"))
    print("bwd_cf %d x %d %s (P = %d, K = %d): dX%s, dW, red %s" % (co, ci, name, P, Kp, " (head, tail)" if "tail_from" in kw else "", _fmt(got)))
    assert all(e <= b for e, b in zip(got, bounds)), (got, bounds)
    if kw.get("dead") is not None:                                  # a dead column of X: its dW column keeps its bits, its dX column is zero
        d = kw["dead"]
        assert torch.equal(o["dW"][:, d], o["dW0"][:, d]) and float(o["dX"][:P, d].abs().max()) == 0.0
    if name == "rows-R":                                            # run-to-run identical weight gradient (slabs summed in a fixed order)
        o2 = _cf_outputs(dev, P, co, ci, pitches)
        _cf_run(lib, c, o2, P, co, ci)
        assert torch.equal(o["dW"], o2["dW"]) and torch.equal(o["dX"].view(torch.int32), o2["dX"].view(torch.int32))


@pytest.mark.parametrize("co,ci", SHAPES_CF)
def test_pooled_backward_from_the_input_is_refused_below_the_threshold(dev, co, ci):
    """P = R - 32: pn2_conv1x1_bwd_cf_supported says 0, the call answers PN2_EUNSUPPORTED, nothing is launched and every output
    holds its sentinel / initial bits."""
    lib = _lib.load()
    P = _thr() - 32
    c, _ = C.bwd_cf_case(dev, P, co, ci, 32, 7)
    o = _cf_outputs(dev, P, co, ci, {})
    assert lib.pn2_conv1x1_bwd_cf_supported(P, co, ci, 32) == 0 and lib.pn2_conv1x1_bwd_cf_supported(P + 32, co, ci, 32) == 1
    assert _cf_call(lib, c, o, P, co, ci) == _lib.PN2_EUNSUPPORTED and _last(lib) == ""
    torch.cuda.synchronize()
    assert _cf_untouched(o, ci)


SMALL_CF = [pytest.param(co, ci, n, id="%dx%d-%s" % (co, ci, n)) for co, ci in SHAPES_CF for n in C.SMALL_N]
assert len(SMALL_CF) == 2 * 13


@pytest.mark.parametrize("co,ci,n", SMALL_CF)
def test_pooled_backward_from_the_input_on_a_handful_of_chunks(dev, co, ci, n):
    """PN2_RES_MIN_ROWS = 32 for the call: P = 32 n rows, n from 1 to 2 g + 1 (module docstring)."""
    lib = _lib.load()
    P = 32 * C.small_n(n, min(_cus(dev), 256))
    c, ref = C.bwd_cf_case(dev, P, co, ci, 32, 300 + P % 9973)
    o = _cf_outputs(dev, P, co, ci, dict(ldxo=ci + 4))
    old = _thr()
    _lib.set_option("PN2_RES_MIN_ROWS", 32)
    try:
        _cf_run(lib, c, o, P, co, ci)
    finally:
        _lib.set_option("PN2_RES_MIN_ROWS", old)
    got, bounds = _cf_errors(o, ref, P, co, ci)
    print("bwd_cf %d x %d, %s chunks (P = %d): dX, dW, red %s" % (co, ci, n, P, _fmt(got)))
    assert all(e <= b for e, b in zip(got, bounds)), (got, bounds)


def _lazy_pair(dev, lib, co, P, accumulate, run):
    """`run(coef, lazy)` twice: on a block pn2_bn_bwd_coef wrote beforehand, and with the lazy record.  Asserts the two blocks
    bit-equal, dgamma / dbeta bit-equal and written exactly once in the given accumulate mode, the block within 1e-6 of fp64;
    returns the two results of `run`."""
    rnd = _rnd(dev, 6 + accumulate)
    aff_l = R.draw_affine(rnd, co, co, dev)                         # this layer's own affine block
    gamma = rnd(co) * 0.5 + 1.0
    gamma[::5] *= -1.0
    r01 = rnd(2, co).double() * P ** 0.5
    red_in = R.replicate(r01)
    dg0, db0 = rnd(co), rnd(co)
    out = []
    for lazy_run in (False, True):
        coef, dg, db = torch.zeros(4 * co, device=dev), dg0.clone(), db0.clone()
        if lazy_run:
            z = _lib.BnCoefLazy(red_in.data_ptr(), gamma.data_ptr(), aff_l.data_ptr(), coef.data_ptr(), dg.data_ptr(), db.data_ptr(), accumulate, P, co)
            res = run(coef, ctypes.byref(z))
        else:
            assert lib.pn2_bn_bwd_coef(red_in.data_ptr(), P, co, gamma.data_ptr(), aff_l.data_ptr(), 1, coef.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                       accumulate, _stream()) == 0
            torch.cuda.synchronize()
            res = run(coef, None)
        torch.cuda.synchronize()
        out.append((coef, dg, db, res))
    (coef1, dg1, db1, res1), (coef2, dg2, db2, res2) = out
    assert torch.equal(coef1, coef2) and torch.equal(dg1, dg2) and torch.equal(db1, db2)
    want_g, want_b = (dg0 + r01[1].float(), db0 + r01[0].float()) if accumulate else (r01[1].float(), r01[0].float())
    assert torch.equal(dg2, want_g) and torch.equal(db2, want_b)                            # written exactly once
    a = aff_l.view(4, co)
    blk = R.coef_block(r01[0], r01[1], P, gamma, a[0], a[3])
    assert max(R.rel(coef2.view(4, co)[i], blk[i]) for i in range(4)) <= 1e-6
    return res1, res2


@pytest.mark.parametrize("co,ci", SHAPES_CF)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_pooled_backward_from_the_input_with_the_lazy_coefficient_record(dev, co, ci, accumulate):
    """coef_lazy (cf_prep_kernel realises the block; LAZY_BN = 1 of the training step) against the same call on a block written by
    pn2_bn_bwd_coef: block, dX and dW bit-equal (the slabs are summed in a fixed order), the reductions within their bound, dgamma /
    dbeta written once in both accumulate modes; the results themselves held to fp64 like every other case."""
    lib = _lib.load()
    P = _thr() + 64

    def run(coef, lazy):
        c, ref = C.bwd_cf_case(dev, P, co, ci, 64, 500 + ci, coef=coef, arg_mode="planted", ldo=co + 8)
        o = _cf_outputs(dev, P, co, ci, {})
        _cf_run(lib, c, o, P, co, ci, lazy)
        return c, ref, o
    (c1, ref, o1), (_, _, o2) = _lazy_pair(dev, lib, co, P, accumulate, run)
    assert torch.equal(o1["dX"].view(torch.int32), o2["dX"].view(torch.int32)) and torch.equal(o1["dW"], o2["dW"])
    for o in (o1, o2):
        got, bounds = _cf_errors(o, ref, P, co, ci)
        print("bwd_cf %d x %d lazy, accumulate %d: dX, dW, red %s" % (co, ci, accumulate, _fmt(got)))
        assert all(e <= b for e, b in zip(got, bounds)), (got, bounds)


def test_pooled_backward_from_the_input_with_pool_cf_1_takes_128x96_only(dev):
    """PN2_POOL_CF = 1: 128 x 64 is refused (nothing touched), 128 x 96 runs as before."""
    lib = _lib.load()
    P = _thr()
    old = _lib.options()["PN2_POOL_CF"]
    _lib.set_option("PN2_POOL_CF", 1)
    try:
        c, _ = C.bwd_cf_case(dev, P, 128, 64, 32, 8)
        o = _cf_outputs(dev, P, 128, 64, {})
        assert lib.pn2_conv1x1_bwd_cf_supported(P, 128, 64, 32) == 0
        assert _cf_call(lib, c, o, P, 128, 64) == _lib.PN2_EUNSUPPORTED and _last(lib) == ""
        torch.cuda.synchronize()
        assert _cf_untouched(o, 64)
        c, ref = C.bwd_cf_case(dev, P, 128, 96, 32, 9)
        o = _cf_outputs(dev, P, 128, 96, {})
        _cf_run(lib, c, o, P, 128, 96)
    finally:
        _lib.set_option("PN2_POOL_CF", old)
    got, bounds = _cf_errors(o, ref, P, 128, 96)
    print("bwd_cf 128 x 96 with POOL_CF = 1: dX, dW, red %s" % _fmt(got))
    assert all(e <= b for e, b in zip(got, bounds)), (got, bounds)


# =============================================================================================== pn2_conv1x1_bwd_first + wgrad_cf(dZ = NULL)

def _first_outputs(dev, co, ci, N0, seed=2):
    rnd = _rnd(dev, seed)
    dW, dW0 = R.framed(co, ci, ci + 4, rnd)
    dWf, dWf0 = R.framed(ci, N0, N0 + 5, rnd)
    return dict(dW=dW, dW0=dW0, lddw=ci + 4, dWf=dWf, dWf0=dWf0, lddwf=N0 + 5, red=torch.zeros(R.STAT_REPLICAS * 2 * ci, device=dev, dtype=torch.float64),
                scratch=_scratch(int(_lib.load().pn2_conv1x1_wgrad_cf_scratch_bytes()), dev, 0))      # zeroed: the contract of cf_scratch


def _first_call(lib, c, o, P, co, ci, lazy=None):
    lib.pn2_clear_last_kernel()
    dZ = c["keep"][0]
    return lib.pn2_conv1x1_bwd_first(dZ.data_ptr(), c["ldc"], c["Y"].data_ptr(), c["ldc"], c["coef"].data_ptr(), c["W"].data_ptr(), c["ldw"],
                                     c["Yp"].data_ptr(), c["ldp"], c["affp"].data_ptr(), o["red"].data_ptr(), o["dW"].data_ptr(), o["lddw"],
                                     c["X0"].data_ptr(), c["ld0"], c["N0"], o["scratch"].data_ptr(), P, co, ci, lazy, _stream())


def _first_run(lib, c, o, P, co, ci, lazy=None):
    """pn2_conv1x1_bwd_first, then the first layer's pn2_conv1x1_wgrad_cf without dZ on the same scratch."""
    assert lib.pn2_conv1x1_bwd_first_supported(P, co, ci, c["N0"]) == 1
    rc = _first_call(lib, c, o, P, co, ci, lazy)
    assert rc == 0, rc
    assert _is(_last(lib), FUSE0_KERNEL), _last(lib)
    rc = lib.pn2_conv1x1_wgrad_cf(None, 0, c["coef0"].data_ptr(), c["X0"].data_ptr(), c["ld0"], c["W0"].data_ptr(), c["ldw0"], c["b0"].data_ptr(),
                                  o["scratch"].data_ptr(), o["dWf"].data_ptr(), o["lddwf"], P, ci, c["N0"], None, _stream())
    assert rc == 0, rc
    assert _is(_last(lib), r"wgrad_first_cf_kernel<\s*%d," % (ci // 16)), _last(lib)
    torch.cuda.synchronize()


def _first_untouched(o):
    return torch.equal(o["dW"], o["dW0"]) and float(o["red"].abs().max()) == 0.0 and int(o["scratch"][:-GUARD_BYTES].max()) == 0


def _first_errors(o, ref, co, ci, N0):
    """(dW, red0, red1, dW0) against fp64; dW's frame, dW0's frame (columns >= N0 among it) and the scratch's end checked."""
    R.check_frame(o["dW"], o["dW0"], co, ci, "dW")
    R.check_frame(o["dWf"], o["dWf0"], ci, N0, "the first layer's dW")
    _scratch_intact(o["scratch"], "cf_scratch")
    red = _stat_sums(o["red"], ci)
    return [R.rel(o["dW"][:co, :ci], o["dW0"][:co, :ci].double() + ref["dW"]), R.rel(red[0], ref["r0"]), R.rel(red[1], ref["r1"]),
            R.rel(o["dWf"][:ci, :N0], o["dWf0"][:ci, :N0].double() + ref["dW0"])]


def _first_rows(name, thr, g):
    k = thr // (32 * g) + 1                                         # 64 (k g / 2) + 64: k trips for every workgroup and a tile more
    return {"R": (thr, None), "R+64": (thr + 64, thr), "trips+1-tile": (64 * (k * g // 2) + 64, None)}[name]


FIRST_PARAMS = [pytest.param(co, ci, rows, 12, 12, id="%dx%d-%s" % (co, ci, rows)) for co, ci in SHAPES_FIRST for rows in ("R", "R+64", "trips+1-tile")] + \
               [pytest.param(co, ci, "R", N0, ld0, id="%dx%d-N0=%d-ld0=%d" % (co, ci, N0, ld0)) for co, ci in SHAPES_FIRST for N0 in (1, 3, 6, 9, 12)
                for ld0 in (12, 16)]
assert len(FIRST_PARAMS) == 2 * (3 + 10)


@pytest.mark.parametrize("co,ci,rows,N0,ld0", FIRST_PARAMS)
def test_fused_backward_with_the_first_layers_sums_at_its_seams(dev, co, ci, rows, N0, ld0):
    """Row counts R, R + 64 (the last tile's rows weigh 32 x) and k trips for every workgroup plus one tile (g = the CU count,
    launch_split_bwd_res's cap); N0 = 1 .. 12 with ld0 = 12 (zero pad columns) and ld0 = 16 (NaN in columns 12 .. 15), dZ / Y /
    prev_Y at pitches beyond their widths in every other case."""
    lib = _lib.load()
    P, tail = _first_rows(rows, _thr(), _cus(dev))
    c, ref = C.first_case(dev, P, co, ci, N0, ld0, 700 + co + N0 + ld0 + len(rows), tail_from=tail, wide=(N0 + ld0 // 4) % 2 == 1)
    o = _first_outputs(dev, co, ci, N0)
    _first_run(lib, c, o, P, co, ci)
    got = _first_errors(o, ref, co, ci, N0)
    print("bwd_first %d x %d, P = %d (%s), N0 = %d, ld0 = %d: dW, red, first layer's dW %s" % (co, ci, P, rows, N0, ld0, _fmt(got)))
    assert max(got) <= C.TOL, got


@pytest.mark.parametrize("co,ci", SHAPES_FIRST)
def test_fused_backward_with_the_first_layers_sums_is_refused_outside_its_rows(dev, co, ci):
    """P = R - 64 and P = R + 32 (no whole number of 64-row tiles): PN2_EUNSUPPORTED, nothing launched, nothing touched."""
    lib = _lib.load()
    for P in (_thr() - 64, _thr() + 32):
        c, _ = C.first_case(dev, P, co, ci, 6, 12, 11)
        o = _first_outputs(dev, co, ci, 6)
        assert lib.pn2_conv1x1_bwd_first_supported(P, co, ci, 6) == 0
        assert _first_call(lib, c, o, P, co, ci) == _lib.PN2_EUNSUPPORTED and _last(lib) == ""
        torch.cuda.synchronize()
        assert _first_untouched(o)
    assert lib.pn2_conv1x1_bwd_first_supported(_thr(), co, ci, 6) == 1 and lib.pn2_conv1x1_bwd_first_supported(_thr(), co, ci, 13) == 0


SMALL_FIRST = [pytest.param(co, ci, n, id="%dx%d-%s" % (co, ci, n)) for co, ci in SHAPES_FIRST for n in C.SMALL_N]
assert len(SMALL_FIRST) == 2 * 13


@pytest.mark.parametrize("co,ci,n", SMALL_FIRST)
def test_fused_backward_with_the_first_layers_sums_on_a_handful_of_tiles(dev, co, ci, n):
    """PN2_RES_MIN_ROWS = 32 for the calls: P = 64 n rows, n from 1 to 2 g + 1 tiles, N0 = 9 at ld0 = 12."""
    lib = _lib.load()
    P = 64 * C.small_n(n, _cus(dev))
    c, ref = C.first_case(dev, P, co, ci, 9, 12, 800 + P % 9973, wide=True)
    o = _first_outputs(dev, co, ci, 9)
    old = _thr()
    _lib.set_option("PN2_RES_MIN_ROWS", 32)
    try:
        _first_run(lib, c, o, P, co, ci)
    finally:
        _lib.set_option("PN2_RES_MIN_ROWS", old)
    got = _first_errors(o, ref, co, ci, 9)
    print("bwd_first %d x %d, %s tiles (P = %d): dW, red, first layer's dW %s" % (co, ci, n, P, _fmt(got)))
    assert max(got) <= C.TOL, got


@pytest.mark.parametrize("co,ci", SHAPES_FIRST)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_fused_backward_with_the_first_layers_sums_and_the_lazy_coefficient_record(dev, co, ci, accumulate):
    """coef_lazy against the same call on a block written by pn2_bn_bwd_coef: block bit-equal, dgamma / dbeta written once, every
    result (their atomics land in another order) within its bound of fp64."""
    lib = _lib.load()
    P = _thr() + 64

    def run(coef, lazy):
        c, ref = C.first_case(dev, P, co, ci, 6, 12, 900 + co, coef=coef)
        o = _first_outputs(dev, co, ci, 6)
        _first_run(lib, c, o, P, co, ci, lazy)
        return ref, o
    (ref, o1), (_, o2) = _lazy_pair(dev, lib, co, P, accumulate, run)
    for o in (o1, o2):
        got = _first_errors(o, ref, co, ci, 6)
        print("bwd_first %d x %d lazy, accumulate %d: dW, red, first layer's dW %s" % (co, ci, accumulate, _fmt(got)))
        assert max(got) <= C.TOL, got


# =============================================================================================== pn2_conv1x1_wgrad_cf with dZ

WGRAD_MS, WGRAD_NS, WGRAD_PS = tuple(range(16, 129, 16)), (1, 3, 4, 5, 9, 12, 15), (1, 3, 127, 128, 129, 511, 512, 513)


def _wgrad_cf_case(lib, dev, P, M, N, ldx, kind, seed):
    c, ref = C.wgrad_cf_case(dev, P, M, N, ldx, M + 4, seed, coef=kind)
    dW, dW0 = R.framed(M, N, N + 2, _rnd(dev, seed + 1))
    scratch = _scratch(int(lib.pn2_conv1x1_wgrad_cf_scratch_bytes()), dev, 0)
    lib.pn2_clear_last_kernel()
    rc = lib.pn2_conv1x1_wgrad_cf(c["dZ"].data_ptr(), c["ldz"], c["coef"].data_ptr(), c["X"].data_ptr(), ldx, c["W"].data_ptr(), c["ldw"],
                                  c["bias"].data_ptr(), scratch.data_ptr(), dW.data_ptr(), N + 2, P, M, N, None, _stream())
    assert rc == 0, rc
    assert _is(_last(lib), r"wgrad_first_cf_kernel<\s*%d," % (M // 16)), _last(lib)
    torch.cuda.synchronize()
    R.check_frame(dW, dW0, M, N, "dW")
    _scratch_intact(scratch, "scratch")
    want = dW0[:M, :N].double() + ref["dW"]
    return R.rel(dW[:M, :N], want), C.bound(kind, R.rel(dW0[:M, :N].double() + ref["f32"]["dW"].double(), want))


WGRAD_PARAMS = [pytest.param(M, N, id="%dx%d" % (M, N)) for M in WGRAD_MS for N in WGRAD_NS]
assert len(WGRAD_PARAMS) == 56


@pytest.mark.parametrize("M,N", WGRAD_PARAMS)
def test_first_layer_closed_form_weight_gradient_on_small_and_odd_shapes(dev, M, N):
    """pn2_conv1x1_wgrad_cf with dZ on P = 1 .. 513 rows (around the 4-row MFMA step, the 128-row trip of a workgroup and the
    512 rows per workgroup of the grid), ldx = round4(N) and round4(N) + 4 with NaN from column N on, ldz = M + 4, input columns
    with non-zero means; the random block on every case and the self-consistent one where mlp_cf_ref.wgrad_cf_kinds gives it.  The scratch
    is fresh and zeroed for every call (the contract; a second call on the dirty scratch is not made)."""
    lib = _lib.load()
    errs = []
    for i, P in enumerate(WGRAD_PS):
        for ldx in (R.round4(N), R.round4(N) + 4):
            for kind in C.wgrad_cf_kinds(P, N):
                e, b = _wgrad_cf_case(lib, dev, P, M, N, ldx, kind, 1000 + 7 * M + N + 131 * i + ldx)
                assert e <= b, (P, ldx, kind, e, b)
                errs.append(e)
    print("wgrad_cf %d x %d, P = 1 .. 513: dW %s (largest of %d calls)" % (M, N, _fmt([max(errs)]), len(errs)))


@pytest.mark.parametrize("kind", ["random", "self"])
def test_first_layer_closed_form_weight_gradient_with_the_grid_cap_binding(dev, kind):
    """One row count beyond 512 CF_WGS_PER_CU CUs: the grid is capped and every wave takes more than one trip, the last ragged."""
    lib = _lib.load()
    P = 512 * _lib.options()["PN2_CF_WGS_PER_CU"] * _cus(dev) + 513
    e, b = _wgrad_cf_case(lib, dev, P, 32, 9, 12, kind, 1500)
    print("wgrad_cf 32 x 9, P = %d (%s block): dW %s" % (P, kind, _fmt([e])))
    assert e <= b, (e, b)


def test_first_layer_closed_form_weight_gradient_refuses_other_shapes(dev):
    """N = 16 and M = 24: PN2_EUNSUPPORTED, nothing launched, dW untouched."""
    lib = _lib.load()
    for M, N in ((16, 16), (24, 9)):
        rnd = _rnd(dev, 3)
        X, dZ, W, b, coef = rnd(64, 16), rnd(64, 32), rnd(32, 16), rnd(32), R.draw_coef(rnd, 32, 32, dev)
        dW, dW0 = R.framed(32, 16, 16, rnd)
        scratch = _scratch(int(lib.pn2_conv1x1_wgrad_cf_scratch_bytes()), dev, 0)
        lib.pn2_clear_last_kernel()
        rc = lib.pn2_conv1x1_wgrad_cf(dZ.data_ptr(), 32, coef.data_ptr(), X.data_ptr(), 16, W.data_ptr(), 16, b.data_ptr(), scratch.data_ptr(), dW.data_ptr(),
                                      16, 64, M, N, None, _stream())
        torch.cuda.synchronize()
        assert rc == _lib.PN2_EUNSUPPORTED and _last(lib) == "" and torch.equal(dW, dW0) and int(scratch[:-GUARD_BYTES].max()) == 0
