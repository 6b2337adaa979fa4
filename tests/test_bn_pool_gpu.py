"""GPU: the small kernels between the GEMMs, kernel by kernel through the C ABI, against the fp64 statements of
tests/bn_pool_ref.py -- pn2_bn_relu_max, pn2_bn_pool_select, the {value, row} records of pn2_conv1x1_fwd_pool,
pn2_pool_bwd_reduce / _ld / _rec, pn2_relu_bwd_reduce, pn2_bn_finalize / pn2_bn_bwd_coef as stand-alone launches, and the
PointNet v1 / DenseCls relatives at their own seams.

The forward kernels run on LATTICE operands (every fma exact in float32): out and arg are compared bit for bit, with ties
planted across row-lanes, across the four waves of the ksplit form, in all-equal and all-non-positive groups.  The
reductions run on random operands whose Y holds 1e30 wherever arg does not point; dZp / dZ are exact (a copy or a zero),
red0 is exact (dyadic dOut) and red1 is held to bounds DERIVED in bn_pool_ref's docstring by counting float32 roundings --
3.01 u sum |dZ xhat| on the gather branch, 1.01 u sum |dZ| (6 |xhat| + (|out| + |beta|) / |gamma|) on the `out` branch -- per
channel, with the branch known from its gamma and beta.  tests/test_bn_pool_ref_cpu.py shows on the same operand sets that a
float32 emulation stays inside these bounds and that seven mutants of it do not.

Every output sits in guard rows and columns (mlp_ref: GUARDS) at a pitch above round4(C); every case asserts its premise
(which form the host-side rule picks, that the grid cap is exceeded) from the device's compute-unit count, so a case cannot
silently move to another branch.  Each test prints its measured error in units of its bound.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from pointnet12_amd import _lib

import bn_pool_ref as B
import mlp_ref as R

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
i32, f32, f64 = np.int32, np.float32, np.float64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _p(t):
    return None if t is None else t.data_ptr()


def _red_sum(red, C):
    return _n(red).reshape(R.STAT_REPLICAS, 2, C).sum(0)


def _zeros_red(C, dev):
    return torch.zeros(R.STAT_REPLICAS * 2 * C, device=dev, dtype=torch.float64)


def _units(err, bound):
    """Largest error in units of its bound (0 / 0 = 0: an exact sum with a zero bound)."""
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())


# =============================================================================================== (a) pn2_bn_relu_max

def _run_relu_max(lib, dev, c, arg_null=False, lazy=None, aff=None):
    G, K, C = c["G"], c["K"], c["C"]
    ldy, ldo = R.round4(C) + 4, R.round4(C) + 8
    Y = _t(B.rows(G * K, C, ldy, c["Y"].reshape(G * K, C)), dev)
    aff = _t(c["aff"], dev) if aff is None else aff
    out, arg = R.guarded(G, ldo, dev), R.guarded(G, ldo, dev)
    rc = lib.pn2_bn_relu_max(Y.data_ptr(), ldy, aff.data_ptr(), G, K, C, out.data_ptr(), ldo, None if arg_null else arg.data_ptr(), lazy, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    R.check_guards(out, G, C, "out")
    if not arg_null:
        R.check_guards(arg, G, C, "arg")
    return _n(out[:G, :C]), _n(arg.view(torch.int32)[:G, :C])


@pytest.mark.parametrize("index", range(len(B.relu_max_cases(256))), ids=["%s-%d" % c[:2] for c in B.relu_max_cases(256)])
def test_bn_relu_max_is_exact_on_the_lattice(dev, index):
    """(a) every form and lane geometry of bn_relu_max_kernel, bit-equal to max_k max(z_k, 0) and the first k attaining it.  The
    table depends on the compute-unit count (grid caps); its length does not."""
    lib, cus = _lib.load(), _cus(dev)
    form, seed, G, K, C = B.relu_max_cases(cus)[index]
    got_form, trips = B.relu_max_form(cus, G, K, C)
    assert got_form == form, (form, got_form)                       # the premise: the host-side rule takes this form
    if seed in (320, 373) or seed >= 440:
        assert trips >= 2, "G = %d does not exceed the grid cap" % G
    if seed == 372:
        assert K >= 32 and G * B.lane_geometry(C)[2] > 4096
    c = B.lattice_case(seed, G, K, C)
    arg_null = seed == 300
    out, arg = _run_relu_max(lib, dev, c, arg_null=arg_null)
    bad_o = int((out.view(i32) != c["out"].view(i32)).sum())
    bad_a = 0 if arg_null else int((arg != c["arg"]).sum())
    print("bn_relu_max %s G=%d K=%d C=%d (LPR %d, RPW %d, gx %d; %d trips): %d / %d wrong out, %d wrong arg" %
          ((form, G, K, C) + B.lane_geometry(C) + (trips, bad_o, out.size, bad_a)))
    assert bad_o == 0 and bad_a == 0


def _lazy_pair(lib, dev, s, run):
    """run(aff, lazy) twice -- on a block written beforehand by pn2_bn_finalize, and with the pn2_bn_lazy prologue -- from sums
    laid out by mlp_ref.replicate.  Returns [(result, aff, rmean, rvar, nbt)] of the two runs."""
    P, C = s["P"], s["C"]
    stats = R.replicate(torch.stack([_t(s["s1"], dev), _t(s["s2"], dev)]))
    gamma, beta = _t(s["gamma"], dev), _t(s["beta"], dev)
    runs = []
    for lazy_run in (False, True):
        aff = torch.zeros(4 * R.round4(C), device=dev)
        rm, rv, nbt = _t(s["rmean"], dev), _t(s["rvar"], dev), torch.zeros(1, device=dev, dtype=torch.int64)
        if lazy_run:
            z = _lib.BnLazy(stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(),
                            aff.data_ptr(), P, C)
            res = run(aff, ctypes.byref(z))
        else:
            assert lib.pn2_bn_finalize(stats.data_ptr(), P, C, gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, 1, rm.data_ptr(), rv.data_ptr(),
                                       nbt.data_ptr(), aff.data_ptr(), _stream()) == 0
            res = run(aff, None)
        torch.cuda.synchronize()
        runs.append((res, _n(aff), _n(rm), _n(rv), int(nbt)))
    return runs


def _check_lazy_pair(s, runs, what):
    (res1, aff1, rm1, rv1, nbt1), (res2, aff2, rm2, rv2, nbt2) = runs
    for a, b in zip(res1, res2):
        assert np.array_equal(a.view(i32), b.view(i32)), what
    assert np.array_equal(aff1.view(i32), aff2.view(i32)), what
    assert np.array_equal(rm1, rm2) and np.array_equal(rv1, rv2) and nbt1 == 1 and nbt2 == 1, (what, nbt1, nbt2)
    # updated exactly ONCE although every workgroup ran the prologue: one step of the fp64 statement, within an ulp
    T = torch.from_numpy
    rm_ref, rv_ref = R.running_stats(T(s["s1"]), T(s["s2"]), s["P"], float(np.float32(MOMENTUM)), T(s["rmean"]), T(s["rvar"]))
    e = max(float(B.ulps(rm2, rm_ref.numpy()).max()), float(B.ulps(rv2, rv_ref.numpy()).max()))
    print("%s: lazy == eager bit for bit; running statistics %.1f ulp from one fp64 step" % (what, e))
    assert e <= 1.0


@pytest.mark.parametrize("G,K,C", [(67, 1, 260), (3, 33, 64)])
def test_bn_relu_max_with_the_lazy_block(dev, G, K, C):
    """(a) pn2_bn_lazy in the K == 1 form (34 workgroups) and in the ksplit form (3): out, arg and the block bit-equal to
    pn2_bn_finalize + the eager call, running statistics updated once, num_batches_tracked + 1."""
    lib = _lib.load()
    assert B.relu_max_form(_cus(dev), G, K, C)[0] == ("k1" if K == 1 else "ksplit")
    c = B.lattice_case(600 + K, G, K, C)
    s = B.stats_case(601 + K, G * K, C)
    runs = _lazy_pair(lib, dev, s, lambda aff, lazy: _run_relu_max(lib, dev, c, lazy=lazy, aff=aff))
    _check_lazy_pair(s, runs, "bn_relu_max G=%d K=%d C=%d" % (G, K, C))


# =============================================================================================== (b) pn2_bn_pool_select

def _run_pool_select(lib, dev, c, lazy=None, aff=None):
    G, C = c["G"], c["C"]
    ldo, off = C + 16, 8                                            # columns [8, 8 + C) of a wider matrix
    rec = _t(c["rec"], dev)
    aff = _t(c["aff"], dev) if aff is None else aff
    out, arg = R.guarded(G, ldo, dev), R.guarded(G, ldo, dev)
    rc = lib.pn2_bn_pool_select(rec.data_ptr(), aff.data_ptr(), G, C, out.data_ptr() + 4 * off, ldo, arg.data_ptr() + 4 * off, lazy, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf, what in ((out, "out"), (arg, "arg")):
        bits = buf.view(torch.int32)
        assert bool((bits[G:] == R.SENTINEL).all()) and bool((bits[:G, :off] == R.SENTINEL).all()) and bool((bits[:G, off + C:] == R.SENTINEL).all()), \
            "%s: written outside its column slice" % what
    return _n(out[:G, off:off + C]), _n(arg.view(torch.int32)[:G, off:off + C])


@pytest.mark.parametrize("index", range(5), ids=["%d-C%d" % (c[0], c[2]) for c in B.select_cases(256)])
def test_bn_pool_select_is_exact_on_drawn_records(dev, index):
    """(b) drawn {value, row} records: out = relu(bn(value)) bit for bit, arg = the recorded row, row 0 under a zero scale
    whatever the record holds; as a column slice of a wider matrix.  The last case's G is the first for which the quads
    G C / 4 exceed the bounded grid of 256 * 8 * CUs threads (the grid-stride loop's second trip)."""
    lib, cus = _lib.load(), _cus(dev)
    seed, G, C = B.select_cases(cus)[index]
    if index == 4:
        assert G * (C // 4) > 256 * 8 * cus
    c = B.record_case(seed, G, 64, C)
    assert bool((c["scale"] == 0).any()) and bool((c["scale"] < 0).any()) and bool((c["row"][:, c["scale"] == 0] != 0).any())
    out, arg = _run_pool_select(lib, dev, c)
    bad_o, bad_a = int((out.view(i32) != c["out"].view(i32)).sum()), int((arg != c["arg"]).sum())
    print("bn_pool_select G=%d C=%d: %d / %d wrong out, %d wrong arg" % (G, C, bad_o, out.size, bad_a))
    assert bad_o == 0 and bad_a == 0


def test_bn_pool_select_with_the_lazy_block(dev):
    lib = _lib.load()
    G, C = 37, 96
    c = B.record_case(537, G, 64, C)
    s = B.stats_case(538, G * 64, C)
    runs = _lazy_pair(lib, dev, s, lambda aff, lazy: _run_pool_select(lib, dev, c, lazy=lazy, aff=aff))
    _check_lazy_pair(s, runs, "bn_pool_select G=%d C=%d" % (G, C))


# =============================================================================================== (c) records of pn2_conv1x1_fwd_pool

def _y_tol(K):
    return 2e-6 * max(1.0, K ** 0.5 / 8)                            # the bound tests/test_mlp_seams_gpu.py holds Y to


def _fwd_pool(lib, dev, P, K, N, Kp, seed, with_y):
    # Y in guard columns too where the kernel takes a pitch (the register-stationary forward wants ldy == N)
    c, ref = R.fixed_forward_case(dev, P, K, N, seed, affine=True, ldy=R.round4(N) + (4 if with_y else 0))
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    gamma = torch.randn(N, device=dev, generator=g) * 0.5 + 1.0
    gamma[::3] *= -1.0
    G = P // Kp
    Yb = R.guarded(P, c["ldy"], dev) if with_y else None
    ws = torch.full((2 * G * N + 64,), R.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    stats = torch.zeros(R.STAT_REPLICAS * 2 * N, device=dev, dtype=torch.float64)
    lib.pn2_clear_last_kernel()
    rc = lib.pn2_conv1x1_fwd_pool(c["X"].data_ptr(), c["ldx"], c["aff"].data_ptr(), c["W"].data_ptr(), c["ldw"], c["bias"].data_ptr(), _p(Yb),
                                  c["ldy"], P, K, N, stats.data_ptr(), Kp, gamma.data_ptr(), ws.data_ptr(), None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    name = lib.pn2_last_kernel()
    assert bool((ws.view(torch.int32)[2 * G * N:] == R.SENTINEL).all()), "records written behind pool_ws"
    rec = ws[:2 * G * N].view(G, N, 2)
    return c, ref, _n(gamma), Yb, _n(rec[..., 0].contiguous()), _n(rec[..., 1].contiguous().view(torch.int32)), (name.decode() if name else "")


def _first_extreme(Yg, gamma):
    """Yg [G, Kp, N] -> (the column extreme over the group's rows: the minimum where gamma < 0, the maximum elsewhere; the first
    row attaining it)."""
    s = np.where(gamma < 0, -Yg, Yg)
    k = s.argmax(1)
    return np.take_along_axis(Yg, k[:, None, :], 1)[:, 0], k


@pytest.mark.parametrize("K,N,Kp", [(64, 64, 16), (64, 64, 32), (64, 64, 64), (32, 128, 32)])
def test_fwd_pool_records_are_the_extremes_of_the_y_it_wrote(dev, K, N, Kp):
    """(c) the weight-resident forward at the smallest row count it accepts: each record's value is, bit for bit, the column
    extreme over the group's rows of the Y the same call wrote (the minimum where gamma < 0), its row the first attaining it;
    Y itself within the forward's bound of fp64."""
    lib = _lib.load()
    thr = _lib.options()["PN2_RES_MIN_ROWS"]
    step = 32 * Kp // math.gcd(32, Kp)
    P = -(-thr // step) * step
    c, ref, gamma, Yb, val, row, name = _fwd_pool(lib, dev, P, K, N, Kp, 700 + K + N + Kp, True)
    assert "fwd_res_kernel<" in name, name
    R.check_guards(Yb, P, N, "Y")
    Y = _n(Yb[:P, :N])
    e_y = R.rel(Yb[:P, :N], ref["Y"])
    ext, k = _first_extreme(Y.reshape(P // Kp, Kp, N), gamma)
    bad_v, bad_k = int((val.view(i32) != ext.view(i32)).sum()), int((row != k).sum())
    print("fwd_pool %d -> %d, Kpool %d, P = %d [%s]: Y %.2e (bound %.1e); %d / %d wrong values, %d wrong rows" %
          (K, N, Kp, P, name[:40], e_y, _y_tol(K), bad_v, val.size, bad_k))
    assert bool((gamma < 0).any()) and bool((gamma > 0).any())
    assert e_y <= _y_tol(K) and bad_v == 0 and bad_k == 0


def test_fwd_pool_records_without_y(dev):
    """(c) Y == NULL (the register-stationary forward, 128 -> 256, Kpool = 64 at WIDE_MIN_ROWS): the recorded value within the
    forward's bound of the fp64 extreme, and the fp64 y of the NAMED row within the same bound of that extreme."""
    lib = _lib.load()
    K, N, Kp = 128, 256, 64
    P = -(-_lib.options()["PN2_WIDE_MIN_ROWS"] // Kp) * Kp
    c, ref, gamma, _, val, row, name = _fwd_pool(lib, dev, P, K, N, Kp, 790, False)
    assert "split_nt_kernel<" in name or "regw_nt_kernel<" in name, name
    Yr = _n(ref["Y"]).reshape(P // Kp, Kp, N)
    ext, _ = _first_extreme(Yr, gamma)
    tol = _y_tol(K) * float(np.abs(Yr).max())
    assert int(row.min()) >= 0 and int(row.max()) < Kp
    named = np.take_along_axis(Yr, row[:, None, :].astype(np.int64), 1)[:, 0]
    e_v, e_r = float(np.abs(val - ext).max()), float(np.abs(named - ext).max())
    print("fwd_pool without Y %d -> %d, P = %d [%s]: value %.3f, named row %.3f of the bound" % (K, N, P, name[:40], e_v / tol, e_r / tol))
    assert e_v <= tol and e_r <= tol


# =============================================================================================== (d) pooled reductions

def _check_reduce(c, st, dzp_buf, red, rows_, what):
    C = c["C"]
    R.check_guards(dzp_buf, rows_, C, "dZp of " + what)
    got = _n(dzp_buf[:rows_, :C])
    assert np.array_equal(got.view(i32), st["dZp"].view(i32)), "dZp of %s is not dOut * (out > 0)" % what
    r = _red_sum(red, C)
    e0, e1 = np.abs(r[0] - st["red0"]), np.abs(r[1] - st["red1"])
    assert bool((e0 == 0).all()), "red0 of %s is not the exact sum (worst %.3g)" % (what, e0.max())
    w = e1 / np.maximum(st["b1"], 1e-300)
    w = np.where(e1 == 0, 0.0, w)
    wo, wg = float(w[st["branch"]].max(initial=0.0)), float(w[~st["branch"]].max(initial=0.0))
    assert wo <= 1.0 and wg <= 1.0, "red1 of %s: %.3f (`out` branch), %.3f (gather branch) of the bound" % (what, wo, wg)
    return wo, wg


@pytest.mark.parametrize("seed,G,K,C,C_in", B.reduce_cases())
def test_pooled_reductions(dev, seed, G, K, C, C_in):
    """(d) pn2_pool_bwd_reduce, _ld (dOut as an unaligned column slice of pitch C + 1) and _rec (records in place of Y, zero-scale
    channels recomputed from prev_Y at pitches above C_in) on one operand set."""
    lib = _lib.load()
    if G > 17:
        assert -(-G // 16) > 1024                                   # behind the 1024-workgroup cap: a second trip
    c = B.reduce_case(seed, G, K, C, C_in=C_in)
    c4 = R.round4(C)
    ldo = c4 + (0 if seed % 4 == 1 else 4)                          # guard columns; ldo == round4(C) in a quarter of the cases
    ldy = c4 + 4
    out = _t(B.rows(G, C, ldo, c["out"], pad=B.POISON), dev)        # (nobody may read out's pad columns)
    arg = _t(np.pad(c["arg"], ((0, 0), (0, ldo - C))), dev)
    Y = _t(B.rows(G * K, C, ldy, c["Y"]), dev)
    aff = _t(c["aff"], dev)
    dOut_o = _t(B.rows(G, C, ldo, c["dOut"], pad=B.POISON), dev)
    flat = np.full(G * (C + 1) + 1, B.POISON, f32)
    flat[1:].reshape(G, C + 1)[:, :C] = c["dOut"]
    dOut_s = _t(flat, dev)
    st = B.reduce_statement(c)
    worst = []
    for kind in ("plain", "ld"):
        dzp, red = R.guarded(G, ldo, dev), _zeros_red(C, dev)
        if kind == "plain":
            rc = lib.pn2_pool_bwd_reduce(dOut_o.data_ptr(), ldo, out.data_ptr(), arg.data_ptr(), Y.data_ptr(), ldy, aff.data_ptr(), G, K, C,
                                         dzp.data_ptr(), red.data_ptr(), _stream())
        else:
            rc = lib.pn2_pool_bwd_reduce_ld(dOut_s.data_ptr() + 4, C + 1, out.data_ptr(), ldo, arg.data_ptr(), Y.data_ptr(), ldy, aff.data_ptr(),
                                            G, K, C, dzp.data_ptr(), red.data_ptr(), _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        worst += list(_check_reduce(c, st, dzp, red, G, "pn2_pool_bwd_reduce" + ("_ld" if kind == "ld" else "")))
    # _rec: records in place of Y
    ldw, ldp = C_in + 3, R.round4(C_in) + 4
    W = _t(B.rows(C, C_in, ldw, c["W"], pad=B.POISON), dev)
    prev = np.full((G * K, ldp), B.POISON, f32)
    prev[::K, :C_in] = c["prev0"]
    prev, prev_aff, bias, rec = _t(prev, dev), _t(c["prev_aff"], dev), _t(c["bias"], dev), _t(c["rec"], dev)
    st_r = B.reduce_statement(c, rec=True)
    dzp, red = R.guarded(G, ldo, dev), _zeros_red(C, dev)
    rc = lib.pn2_pool_bwd_reduce_rec(dOut_s.data_ptr() + 4, C + 1, out.data_ptr(), ldo, arg.data_ptr(), rec.data_ptr(), aff.data_ptr(), G, K, C,
                                     dzp.data_ptr(), red.data_ptr(), W.data_ptr(), ldw, bias.data_ptr(), prev.data_ptr(), ldp, prev_aff.data_ptr(),
                                     C_in, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    worst += list(_check_reduce(c, st_r, dzp, red, G, "pn2_pool_bwd_reduce_rec"))
    print("pool_bwd_reduce G=%d K=%d C=%d (ldo %d, C_in %d), red1 in units of its bound [`out` branch, gather branch]: plain %.3f %.3f  "
          "_ld %.3f %.3f  _rec - %.3f" % ((G, K, C, ldo, C_in) + tuple(worst[:4]) + (worst[5],)))


# =============================================================================================== (e) pn2_relu_bwd_reduce

@pytest.mark.parametrize("seed,P,C", B.dense_cases())
def test_dense_relu_reduction(dev, seed, P, C):
    """(e) pn2_relu_bwd_reduce: dZ exact with zero pad columns at ldz > round4(C), the reductions within the same bounds.  The
    largest P sits behind the 512-workgroup cap: a partial second trip, whose prefetch reads clamped rows that must not count."""
    lib = _lib.load()
    if P > 65:
        assert -(-P // 64) > 512 and P % (16 * 512) != 0            # capped grid, and a last trip that is a partial one
    c = B.reduce_case(seed, P, 1, C, dense=True)
    c4 = R.round4(C)
    ldo, ldy, ldz = c4 + 4, c4 + 8, c4 + 4
    out, dOut = _t(B.rows(P, C, ldo, c["out"], pad=B.POISON), dev), _t(B.rows(P, C, ldo, c["dOut"], pad=B.POISON), dev)
    Y, aff = _t(B.rows(P, C, ldy, c["Y"]), dev), _t(c["aff"], dev)
    dZ, red = R.guarded(P, ldz, dev), _zeros_red(C, dev)
    rc = lib.pn2_relu_bwd_reduce(dOut.data_ptr(), ldo, out.data_ptr(), Y.data_ptr(), ldy, aff.data_ptr(), P, C, dZ.data_ptr(), ldz, red.data_ptr(),
                                 _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    wo, wg = _check_reduce(c, B.reduce_statement(c), dZ, red, P, "pn2_relu_bwd_reduce")
    print("relu_bwd_reduce P=%d C=%d, red1 in units of its bound: `out` branch %.3f, gather branch %.3f" % (P, C, wo, wg))


# =============================================================================================== (f) the two blocks, stand-alone

def _block_buf(C, dev):
    """4 * round4(C) + 64 floats of SENTINEL: the kernels write the C real entries of each row, nothing else."""
    return torch.full((4 * R.round4(C) + 64,), R.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _block_of(buf, C, what):
    ld = R.round4(C)
    bits = _n(buf.view(torch.int32))
    blk = bits[:4 * ld].reshape(4, ld)
    assert bool((bits[4 * ld:] == R.SENTINEL).all()) and bool((blk[:, C:] == R.SENTINEL).all()), "%s: written outside its C entries" % what
    assert not bool((blk[:, :C] == R.SENTINEL).any()), "%s: an entry was not written" % what
    return blk[:, :C].view(f32)


@pytest.mark.parametrize("C", [1, 127, 128, 129, 260])
@pytest.mark.parametrize("P", [1, 1000])
def test_bn_finalize_stand_alone(dev, C, P):
    """(f) pn2_bn_finalize: the training block and the running statistics within one ulp of fp64 (P = 1: unbias factor 1; one
    channel whose variance cancels below zero: clamped, invstd = 1 / sqrt(eps)); NULL running statistics / counter; the
    eval-mode block from the running statistics, which it must leave alone."""
    lib = _lib.load()
    s = B.stats_case(800 + C + P, P, C)
    T = torch.from_numpy
    stats = R.replicate(torch.stack([_t(s["s1"], dev), _t(s["s2"], dev)]))
    gamma, beta = _t(s["gamma"], dev), _t(s["beta"], dev)
    eps32, mom32 = float(np.float32(EPS)), float(np.float32(MOMENTUM))        # the kernels receive both as floats
    cc = s["cancel"]
    assert s["s2"][cc] / P - (s["s1"][cc] / P) ** 2 < 0            # the premise of the clamp
    rm_ref, rv_ref = R.running_stats(T(s["s1"]), T(s["s2"]), P, mom32, T(s["rmean"]), T(s["rvar"]))
    blk_ref = R.affine_block(T(s["s1"]), T(s["s2"]), P, T(s["gamma"]), T(s["beta"]), eps32).numpy()
    assert abs(blk_ref[3, cc] * blk_ref[3, cc] * eps32 - 1.0) < 1e-12   # clamped to 0: invstd = 1 / sqrt(eps)
    errs = []
    for with_running in (True, False):
        aff = _block_buf(C, dev)
        rm, rv, nbt = _t(s["rmean"], dev), _t(s["rvar"], dev), torch.full((1,), 41, device=dev, dtype=torch.int64)
        rc = lib.pn2_bn_finalize(stats.data_ptr(), P, C, gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, 1, _p(rm if with_running else None),
                                 _p(rv if with_running else None), _p(nbt if with_running else None), aff.data_ptr(), _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = _block_of(aff, C, "affine")
        errs.append(float(B.ulps(got, blk_ref).max()))
        assert np.array_equal(got[2], s["beta"])
        if with_running:
            errs += [float(B.ulps(_n(rm), rm_ref.numpy()).max()), float(B.ulps(_n(rv), rv_ref.numpy()).max())]
            assert int(nbt) == 42
        else:
            assert np.array_equal(_n(rm), s["rmean"]) and np.array_equal(_n(rv), s["rvar"]) and int(nbt) == 41
    # eval mode: the running statistics are read, not written; stats may be NULL
    aff = _block_buf(C, dev)
    rm, rv, nbt = _t(s["rmean"], dev), _t(s["rvar"], dev), torch.full((1,), 41, device=dev, dtype=torch.int64)
    rc = lib.pn2_bn_finalize(None, P, C, gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, 0, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(),
                             aff.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = _block_of(aff, C, "eval affine")
    errs.append(float(B.ulps(got, B.eval_block(s["gamma"], s["beta"], s["rmean"], s["rvar"], eps32)).max()))
    assert np.array_equal(_n(rm), s["rmean"]) and np.array_equal(_n(rv), s["rvar"]) and int(nbt) == 41
    print("bn_finalize C=%d P=%d, ulps from fp64: block %.1f, running %.1f %.1f, block without running %.1f, eval block %.1f" % ((C, P) + tuple(errs)))
    assert max(errs) <= 1.0, errs


@pytest.mark.parametrize("C", [1, 127, 128, 129, 260])
def test_bn_bwd_coef_stand_alone(dev, C):
    """(f) pn2_bn_bwd_coef: the coefficient block within one ulp of fp64; use_batch_stats = 0 (q1 = q0 = 0 exactly); dgamma /
    dbeta overwritten (accumulate = 0) or added to exactly once (1); dgamma == NULL."""
    lib = _lib.load()
    P = 1000
    s = B.stats_case(900 + C, P, C)
    rng = np.random.default_rng(901 + C)
    T = torch.from_numpy
    mean, invstd = (rng.standard_normal(C) * 0.3).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32)
    aff = _t(B.block(mean, (s["gamma"].astype(f64) * invstd).astype(f32), s["beta"], invstd), dev)
    red = R.replicate(torch.stack([_t(s["r0"], dev), _t(s["r1"], dev)]))
    gamma = _t(s["gamma"], dev)
    ref = R.coef_block(T(s["r0"]), T(s["r1"]), P, T(s["gamma"]), T(mean), T(invstd)).numpy()
    dg0, db0 = rng.standard_normal(C).astype(f32), rng.standard_normal(C).astype(f32)
    r0_32, r1_32 = s["r0"].astype(f32), s["r1"].astype(f32)
    errs = []
    for use_batch, accumulate, with_dg in ((1, 0, True), (1, 1, True), (0, 1, True), (1, 1, False)):
        coef = _block_buf(C, dev)
        dg, db = _t(dg0, dev), _t(db0, dev)
        rc = lib.pn2_bn_bwd_coef(red.data_ptr(), P, C, gamma.data_ptr(), aff.data_ptr(), use_batch, coef.data_ptr(), _p(dg if with_dg else None),
                                 db.data_ptr(), accumulate, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = _block_of(coef, C, "coef")
        want = ref.copy()
        if not use_batch:
            want[1:3] = 0.0
            assert not got[1:3].any()
        errs.append(float(B.ulps(got, want).max()))
        assert np.array_equal(got[3], mean)
        assert np.array_equal(_n(db), db0 + r0_32 if accumulate else r0_32)
        assert np.array_equal(_n(dg), (dg0 + r1_32 if accumulate else r1_32) if with_dg else dg0)
    print("bn_bwd_coef C=%d, ulps from fp64 (batch / accumulate / eval / no dgamma): %s" % (C, " ".join("%.1f" % e for e in errs)))
    assert max(errs) <= 1.0, errs


# =============================================================================================== (g) v1 / DenseCls relatives

@pytest.mark.parametrize("G,K,C", [(3, 1, 3), (3, 63, 13), (3, 65, 20), (2, 65, 3), (65537, 2, 4)])
def test_bn_max_is_exact_on_the_lattice(dev, G, K, C):
    """(g) pn2_bn_max (no ReLU) at K around its 64 row lanes, narrow C at pitches above round4(C), ties planted across lanes
    (k0, k0 + 1, k0 + 5) and across a lane's two visits (K = 65: k0 + 64), and G past the 65 535 grid rows."""
    lib = _lib.load()
    c = B.lattice_case(1000 + G % 100 + K + C, G, K, C, relu=False, tie_step=64 if K == 65 and C == 3 else 5)
    ldy, ldo = R.round4(C) + 4, R.round4(C) + 8
    Y, aff = _t(B.rows(G * K, C, ldy, c["Y"].reshape(G * K, C)), dev), _t(c["aff"], dev)
    out, arg = R.guarded(G, ldo, dev), R.guarded(G, ldo, dev)
    rc = lib.pn2_bn_max(Y.data_ptr(), ldy, aff.data_ptr(), G, K, C, out.data_ptr(), ldo, arg.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    R.check_guards(out, G, C, "out")
    R.check_guards(arg, G, C, "arg")
    o, a = _n(out[:G, :C]), _n(arg.view(torch.int32)[:G, :C])
    bad_o, bad_a = int((o.view(i32) != c["out"].view(i32)).sum()), int((a != c["arg"]).sum())
    print("bn_max G=%d K=%d C=%d: %d / %d wrong out, %d wrong arg" % (G, K, C, bad_o, o.size, bad_a))
    assert bad_o == 0 and bad_a == 0


def test_pool_bwd_reduce_noact_behind_its_grid_cap(dev):
    """(g) pn2_pool_bwd_reduce_noact at C = 13, dOut an unaligned slice of pitch C + 1, G = 4 * 1024 + 3 (a second trip behind the
    1024-workgroup cap).  No mask: dZp = dOut, red1 within the gather-branch bound."""
    lib = _lib.load()
    G, K, C = 4 * 1024 + 3, 2, 13
    assert -(-G // 4) > 1024
    c = B.reduce_case(1100, G, K, C)
    ldo, ldy = R.round4(C) + 4, R.round4(C) + 4
    flat = np.full(G * (C + 1) + 1, B.POISON, f32)
    flat[1:].reshape(G, C + 1)[:, :C] = c["dOut"]
    dOut, arg = _t(flat, dev), _t(np.pad(c["arg"], ((0, 0), (0, ldo - C))), dev)
    Y, aff = _t(B.rows(G * K, C, ldy, c["Y"]), dev), _t(c["aff"], dev)
    dzp, red = R.guarded(G, ldo, dev), _zeros_red(C, dev)
    rc = lib.pn2_pool_bwd_reduce_noact(dOut.data_ptr() + 4, C + 1, arg.data_ptr(), ldo, Y.data_ptr(), ldy, aff.data_ptr(), G, K, C, dzp.data_ptr(),
                                       red.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    R.check_guards(dzp, G, C, "dZp")
    assert np.array_equal(_n(dzp[:G, :C]), c["dOut"])
    d = c["dOut"].astype(f64)
    xh = (c["ystar"].astype(f64) - c["mean"]) * c["invstd"]
    r = _red_sum(red, C)
    b1 = 3.01 * B.U32 * np.abs(d * xh).sum(0) + (G + 8) * B.U64 * (np.abs(d * xh).sum(0) + np.abs(d).sum(0))
    assert np.array_equal(r[0], d.sum(0))
    w = _units(np.abs(r[1] - (d * xh).sum(0)), b1)
    print("pool_bwd_reduce_noact G=%d C=%d: red0 exact, red1 %.3f of its bound" % (G, C, w))
    assert w <= 1.0


@pytest.mark.parametrize("C,rpg", [(13, 1), (13, 300), (260, 1), (260, 300)])
def test_group_colsum_on_narrow_and_ragged_shapes(dev, C, rpg):
    """(g) pn2_group_colsum with lds = C (below the pitch of dZ / Y for C = 13), one row per group and a partial last slab (300 rows:
    one slab of 256 and 44 more), within the bound of an fp32 sum of rows_per_group three-rounding terms."""
    lib = _lib.load()
    G = 3
    c = B.colsum_case(1200 + C + rpg, G, rpg, C)
    P, ld = G * rpg, R.round4(C) + 4
    dZ, Y, coef = _t(B.rows(P, C, ld, c["dZ"]), dev), _t(B.rows(P, C, ld, c["Y"]), dev), _t(c["coef"], dev)
    nbytes = int(lib.pn2_group_colsum_workspace_bytes(P, rpg, C))
    assert nbytes == G * -(-rpg // 256) * R.round4(C) * 4
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    s = torch.full((G * C + 64,), R.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    rc = lib.pn2_group_colsum(dZ.data_ptr(), ld, Y.data_ptr(), ld, coef.data_ptr(), P, rpg, C, s.data_ptr(), C, ws.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((s.view(torch.int32)[G * C:] == R.SENTINEL).all()), "s: written behind its G x C elements"
    w = _units(np.abs(_n(s[:G * C]).reshape(G, C).astype(f64) - c["s"]), c["bound"])
    print("group_colsum C=%d rows_per_group=%d: %.3f of its bound" % (C, rpg, w))
    assert w <= 1.0


@pytest.mark.parametrize("K,G,C", [(1, 67, 13), (3, 23, 260), (5, 13, 13), (3, 43, 13), (5, 27, 260)])
def test_bn_bwd_reduce_noact_dense_with_groups_across_workgroups(dev, K, G, C):
    """(g) pn2_bn_bwd_reduce_noact_dense with P = G K just above 64 and above 128 rows (a workgroup's 64-row range starts in the
    middle of a group), narrow and two-block C, dDense aliased to dZ: dZ and red0 exact, red1 within the three-rounding bound."""
    lib = _lib.load()
    P = G * K
    assert P > 64 and (K == 1 or 64 % K != 0)
    c = B.noact_dense_case(1300 + K + G + C, G, K, C)
    ld = R.round4(C) + 4
    dZ = R.guarded(P, ld, dev)
    dZ[:P] = _t(B.rows(P, C, ld, c["dD"]), dev)                     # dDense lives in dZ's rows: aliased
    dP, arg = _t(B.rows(G, C, ld, c["dP"]), dev), _t(np.pad(c["arg"], ((0, 0), (0, ld - C))), dev)
    Y, aff, red = _t(B.rows(P, C, ld, c["Y"]), dev), _t(c["aff"], dev), _zeros_red(C, dev)
    rc = lib.pn2_bn_bwd_reduce_noact_dense(dZ.data_ptr(), ld, dP.data_ptr(), ld, arg.data_ptr(), ld, Y.data_ptr(), ld, aff.data_ptr(), G, K, C,
                                           dZ.data_ptr(), ld, red.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    bits = dZ.view(torch.int32)
    assert bool((bits[P:] == R.SENTINEL).all()), "dZ: a row >= P was written"
    assert bool((dZ[:P, R.round4(C):] == float(B.POISON)).all()), "dZ: a column >= round4(C) was written"
    assert np.array_equal(_n(dZ[:P, :C]), c["dZ"]) and not bool(_n(dZ[:P, C:R.round4(C)]).any())
    r = _red_sum(red, C)
    assert np.array_equal(r[0], c["red0"])
    w = _units(np.abs(r[1] - c["red1"]), c["b1"])
    print("bn_bwd_reduce_noact_dense G=%d K=%d C=%d: dZ, red0 exact, red1 %.3f of its bound" % (G, K, C, w))
    assert w <= 1.0
