"""GPU: the PointNet v1 entry points (csrc/pointnet_v1.hip, csrc/pointnet_dense.hip, the K-concatenated GEMMs of csrc/mlp.hip) at
the C ABI, on the case tables, operands, bounds and checks of tests/pointnet_v1_kernels_ref.py: channel counts that are no
multiples of 4, pitches that differ from the widths and from each other (NaN behind round4(C) in every input, SENTINEL bits in
every output and behind it), the lane counts and block counts at which point_transform and its dT kernel change form, slabs of
255 / 256 / 257 rows, groups that straddle a workgroup's row range, the grid strides of bn_max and pool_bwd_reduce_noact, planted
ties across the row lanes of bn_max, NaN-filled workspaces, and the refusals of every entry point.

No tolerance here is a literal: ``check_*`` of the reference module hold each output to a bound counted from the operands, to a
bit comparison, or to its SENTINEL frame; tests/test_pointnet_v1_kernels_ref_cpu.py shows that a float32 emulation passes them
and that eleven mutants do not.  Every case prints nothing and copies a few kilobytes (the largest: bn_max at G = 65 539, 4 MB).
"""
import ctypes

import numpy as np
import pytest
import torch

from pointnet12_amd import _lib

import pointnet_v1_kernels_ref as K

pytestmark = pytest.mark.gpu

EINVAL = -1
i32 = np.int32


def _ids(cases):
    return [c[0] for c in cases]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.cpu().numpy()


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _red(C, dev):
    return torch.zeros(K.STAT_REPLICAS * 2 * C, device=dev, dtype=torch.float64)


def _nan_ws(nbytes, dev):
    """A workspace of nbytes NaN-filled bytes ("contents irrelevant") followed by a SENTINEL guard, as float32."""
    n = nbytes // 4
    ws = torch.full((n + 2 * K.MAX_K * 4,), K.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)    # (filled as integers:
    ws[:n] = float("nan")                                                     # SENTINEL is a signalling NaN, a float fill would quiet it)
    return ws


def _ok(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ point_transform

@pytest.mark.parametrize("case", K.transform_cases(), ids=_ids(K.transform_cases()))
def test_point_transform(dev, case):
    _, seed, B, N, k = case
    lib = _lib.load()
    o = K.operands(seed, "transform", B=B, N=N, k=k)
    X, D, T = _t(o["X"], dev), _t(o["D"], dev), _t(o["T"], dev)
    out = _t(K.sentinel(B * N, o["ldo"]), dev)
    _ok(lib.pn2_point_transform(X.data_ptr(), o["ldx"], T.data_ptr(), B, N, k, out.data_ptr(), o["ldo"], _st()))
    bad = K.check_transform(o, _n(out))
    nbytes = int(lib.pn2_point_transform_workspace_bytes(B, N, k))
    assert nbytes == K.point_transform_workspace_bytes(B, N, k)
    for mode in ("both", "dX", "dT"):
        dX = _t(K.sentinel(B * N, o["lddx"]), dev) if mode != "dT" else None
        dTs = [torch.full((B, k, k), float("nan"), device=dev) for _ in range(2)] if mode != "dX" else [None]
        ws = _nan_ws(nbytes, dev) if mode != "dX" else None
        for dT in dTs:
            _ok(lib.pn2_point_transform_bwd(D.data_ptr(), o["ldd"], _p(X) if mode != "dX" else None, o["ldx"], T.data_ptr(), B, N, k, _p(dX),
                                            o["lddx"], _p(dT), _p(ws), _st()))
        got = K.check_transform_bwd(o, None if dX is None else _n(dX), None if dTs[0] is None else _n(dTs[0]), None if ws is None else _n(ws),
                                    None if dTs[0] is None else _n(dTs[1]))
        bad += ["%s: %s" % (mode, b) for b in got]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ bn_max and its backward

@pytest.mark.parametrize("case", K.bn_max_cases(), ids=_ids(K.bn_max_cases()))
def test_bn_max(dev, case):
    _, seed, G, Kk, C, with_arg = case
    lib = _lib.load()
    o = K.operands(seed, "bn_max", G=G, K=Kk, C=C)
    Y, aff = _t(o["Y"], dev), _t(o["aff"], dev)
    out = _t(K.sentinel(G, o["ldo"]), dev)
    arg = _t(K.sentinel(G, o["ldo"]).view(i32), dev) if with_arg else None
    _ok(lib.pn2_bn_max(Y.data_ptr(), o["ldy"], aff.data_ptr(), G, Kk, C, out.data_ptr(), o["ldo"], _p(arg), _st()))
    bad = K.check_bn_max(o, _n(out), None if arg is None else _n(arg))
    assert not bad, bad


@pytest.mark.parametrize("case", K.pool_bwd_cases(), ids=_ids(K.pool_bwd_cases()))
def test_pool_bwd_reduce_noact(dev, case):
    _, seed, G, Kk, C, ldd, ldy, mode = case
    lib = _lib.load()
    o = K.operands(seed, "pool_bwd", G=G, K=Kk, C=C, ld_dout=ldd, ldy=ldy, mode=mode)
    dOut, arg, Y, aff = _t(o["dOut"], dev), _t(o["arg"], dev), _t(o["Y"], dev), _t(o["aff"], dev)
    dzp, red = _t(K.sentinel(G, o["ldo"]), dev), _red(C, dev)
    _ok(lib.pn2_pool_bwd_reduce_noact(dOut.data_ptr(), ldd, arg.data_ptr(), o["ldo"], Y.data_ptr(), ldy, aff.data_ptr(), G, Kk, C, dzp.data_ptr(),
                                      red.data_ptr(), _st()))
    bad = K.check_pool_bwd(o, _n(dzp), _n(red))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the broadcast-concat layer

@pytest.mark.parametrize("case", K.gbias_cases(), ids=_ids(K.gbias_cases()))
def test_conv1x1_fwd_gbias(dev, case):
    _, seed, P, Kk, N, rpg, stats, ldg = case
    lib = _lib.load()
    o = K.operands(seed, "gbias", P=P, K=Kk, N=N, rpg=rpg, ldg=ldg)
    X, W, b, gb = _t(o["X"], dev), _t(o["Wfull"], dev), _t(o["bias"], dev), _t(o["gbias"], dev)
    Y = _t(K.sentinel(P, o["ldy"]), dev)
    st = _red(N, dev) if stats else None
    _ok(lib.pn2_conv1x1_fwd_gbias(X.data_ptr(), o["ldx"], W.data_ptr() + 4 * o["off"], o["ldw"], b.data_ptr(), gb.data_ptr(), ldg, rpg,
                                  Y.data_ptr(), o["ldy"], P, Kk, N, _p(st), _st()))
    bad = K.check_gbias(o, _n(Y), None if st is None else _n(st))
    assert not bad, bad


@pytest.mark.parametrize("case", K.colsum_cases(), ids=_ids(K.colsum_cases()))
def test_group_colsum(dev, case):
    _, seed, G, rpg, C, lds = case
    lib = _lib.load()
    o = K.operands(seed, "colsum", G=G, rpg=rpg, C=C, lds=lds)
    P = o["P"]
    dZ, Y, coef = _t(o["dZ"], dev), _t(o["Y"], dev), _t(o["coef"], dev)
    nbytes = int(lib.pn2_group_colsum_workspace_bytes(P, rpg, C))
    assert nbytes == K.group_colsum_workspace_bytes(P, rpg, C)
    ws = _nan_ws(nbytes, dev)
    outs = []
    for _ in range(2):
        s = torch.full((G * lds + 64,), K.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        _ok(lib.pn2_group_colsum(dZ.data_ptr(), o["ldz"], Y.data_ptr(), o["ldy"], coef.data_ptr(), P, rpg, C, s.data_ptr(), lds, ws.data_ptr(), _st()))
        outs.append(_n(s))
    bad = K.check_colsum(o, outs[0], outs[1])
    if not K.is_sentinel(_n(ws)[nbytes // 4:]).all():
        bad.append("workspace: written behind its %d bytes" % nbytes)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the dense head

def _dense_cases():
    return K.dense_cases(K.NOMINAL_CUS)


@pytest.mark.parametrize("case", _dense_cases(), ids=_ids(_dense_cases()))
def test_bn_bwd_reduce_noact_dense(dev, case):
    _, seed, G, Kk, C = case
    lib = _lib.load()
    o = K.operands(seed, "dense", G=G, K=Kk, C=C)
    dD, dP, arg, Y, aff = (_t(o[k], dev) for k in ("dD", "dP", "arg", "Y", "aff"))
    dZ, red = _t(K.sentinel(o["P"], o["ldz"]), dev), _red(C, dev)
    _ok(lib.pn2_bn_bwd_reduce_noact_dense(dD.data_ptr(), o["ldd"], dP.data_ptr(), o["ldp"], arg.data_ptr(), o["lda"], Y.data_ptr(), o["ldy"],
                                          aff.data_ptr(), G, Kk, C, dZ.data_ptr(), o["ldz"], red.data_ptr(), _st()))
    bad = K.check_dense(o, _n(dZ), _n(red))
    # the aliased form: dDense's own buffer (its rows followed by SENTINEL guard rows) receives dZ
    buf = K.sentinel(o["P"], o["ldd"])
    buf[:o["P"]] = o["dD"]
    buf, red2 = _t(buf, dev), _red(C, dev)
    _ok(lib.pn2_bn_bwd_reduce_noact_dense(buf.data_ptr(), o["ldd"], dP.data_ptr(), o["ldp"], arg.data_ptr(), o["lda"], Y.data_ptr(), o["ldy"],
                                          aff.data_ptr(), G, Kk, C, buf.data_ptr(), o["ldd"], red2.data_ptr(), _st()))
    bad += ["aliased: " + b for b in K.check_dense(o, _n(buf), _n(red2), alias=True)]
    assert not bad, bad


@pytest.mark.parametrize("case", K.multi_cases(), ids=_ids(K.multi_cases()))
def test_multi_source_gemms(dev, case):
    _, seed, P, N, mode = case
    lib = _lib.load()
    o = K.operands(seed, "multi", P=P, N=N, mode=mode)
    Xs = [_t(s[0], dev) for s in o["srcs"]]
    affs = [None if s[3] is None else _t(s[3], dev) for s in o["srcs"]]
    table = _lib.src_table([(x.data_ptr(), s[1], s[2], _p(a), int(s[4])) for x, a, s in zip(Xs, affs, o["srcs"])])
    assert len(table) == K.MULTI_MAX
    W, b = _t(o["Wfull"], dev), _t(o["bias"], dev)
    gb = None if o["gbias"] is None else _t(o["gbias"], dev)
    Y = _t(K.sentinel(P, o["ldy"]), dev)
    st = _red(N, dev) if o["stats"] else None
    _ok(lib.pn2_conv1x1_fwd_multi(table, len(table), W.data_ptr() + 4 * o["off"], o["ldw"], b.data_ptr(), _p(gb), o["ldg"], o["rpg"], Y.data_ptr(),
                                  o["ldy"], P, N, _p(st), _st()))
    dZ, coef = _t(o["dZ"], dev), _t(o["coef"], dev)
    dW, db = torch.zeros(N + 2, o["ldw"], device=dev), torch.zeros(N, device=dev)
    _ok(lib.pn2_conv1x1_wgrad_multi(dZ.data_ptr(), o["ldz"], Y.data_ptr(), o["ldy"], coef.data_ptr(), table, len(table),
                                    dW.data_ptr() + 4 * o["off"], o["ldw"], db.data_ptr(), P, N, _st()))
    dX = [_t(K.sentinel(P, s[1]), dev) for s in o["srcs"]]
    ptrs = (ctypes.c_void_p * len(dX))(*[d.data_ptr() for d in dX])
    lds = (ctypes.c_int * len(dX))(*[s[1] for s in o["srcs"]])
    ks = (ctypes.c_int * len(dX))(*[s[2] for s in o["srcs"]])
    _ok(lib.pn2_conv1x1_dgrad_multi(dZ.data_ptr(), o["ldz"], Y.data_ptr(), o["ldy"], coef.data_ptr(), W.data_ptr() + 4 * o["off"], o["ldw"], ptrs, lds,
                                    ks, len(dX), P, N, _st()))
    bad = K.check_multi(o, _n(Y), None if st is None else _n(st), _n(dW), _n(db), [_n(d) for d in dX])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ refusals

def test_every_checked_precondition_is_refused_without_a_write(dev):
    """PN2_EINVAL for each precondition the entry points check, before any launch: every output still holds its SENTINEL bits."""
    lib, st = _lib.load(), _st()
    buf = lambda n: torch.full((n,), K.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    x, t, out, dx, dt, ws, red = buf(4096), buf(4096), buf(4096), buf(4096), buf(4096), buf(4096), buf(4096)
    P = lambda v: v.data_ptr()
    refused = []

    def no(what, rc):
        refused.append(what)
        assert rc == EINVAL, (what, rc)

    # pn2_point_transform(X, ldx, T, B, N, k, out, ldo) / _bwd(dOut, ldd, X, ldx, T, B, N, k, dX, lddx, dT, workspace)
    for k, why in ((0, "k = 0"), (129, "k = 129")):
        no("transform " + why, lib.pn2_point_transform(P(x), 132, P(t), 1, 2, k, P(out), 132, st))
        no("transform_bwd " + why, lib.pn2_point_transform_bwd(P(x), 132, P(x), 132, P(t), 1, 2, k, P(dx), 132, P(dt), P(ws), st))
    no("transform ldx % 4", lib.pn2_point_transform(P(x), 10, P(t), 1, 2, 5, P(out), 8, st))
    no("transform ldx < round4", lib.pn2_point_transform(P(x), 4, P(t), 1, 2, 5, P(out), 8, st))
    no("transform ldo % 4", lib.pn2_point_transform(P(x), 8, P(t), 1, 2, 5, P(out), 9, st))
    no("transform ldo < round4", lib.pn2_point_transform(P(x), 8, P(t), 1, 2, 5, P(out), 4, st))
    no("transform B = 65536", lib.pn2_point_transform(P(x), 4, P(t), 65536, 1, 3, P(out), 4, st))
    no("transform_bwd B = 65536", lib.pn2_point_transform_bwd(P(x), 4, P(x), 4, P(t), 65536, 1, 3, P(dx), 4, P(dt), P(ws), st))
    no("transform_bwd ldd % 4", lib.pn2_point_transform_bwd(P(x), 10, P(x), 8, P(t), 1, 2, 5, P(dx), 8, P(dt), P(ws), st))
    no("transform_bwd ldd < round4", lib.pn2_point_transform_bwd(P(x), 4, P(x), 8, P(t), 1, 2, 5, P(dx), 8, P(dt), P(ws), st))
    no("transform_bwd lddx < round4", lib.pn2_point_transform_bwd(P(x), 8, P(x), 8, P(t), 1, 2, 5, P(dx), 4, P(dt), P(ws), st))
    no("transform_bwd dX and dT NULL", lib.pn2_point_transform_bwd(P(x), 8, P(x), 8, P(t), 1, 2, 5, None, 8, None, P(ws), st))
    # (dX is given too: it must not have been launched by the time the dT half is refused)
    no("transform_bwd dT without workspace", lib.pn2_point_transform_bwd(P(x), 8, P(x), 8, P(t), 1, 2, 5, P(dx), 8, P(dt), None, st))
    no("transform_bwd dT without X", lib.pn2_point_transform_bwd(P(x), 8, None, 8, P(t), 1, 2, 5, P(dx), 8, P(dt), P(ws), st))
    no("transform_bwd dT with ldx < round4", lib.pn2_point_transform_bwd(P(x), 8, P(x), 4, P(t), 1, 2, 5, P(dx), 8, P(dt), P(ws), st))
    # pn2_bn_max(Y, ldy, affine, G, K, C, out, ldo, arg) / pn2_pool_bwd_reduce_noact(dOut, ld_dout, arg, ldo, Y, ldy, affine, G, K, C, dZp, red)
    no("bn_max ldy % 4", lib.pn2_bn_max(P(x), 10, P(t), 2, 2, 5, P(out), 8, P(dx), st))
    no("bn_max ldo < round4", lib.pn2_bn_max(P(x), 8, P(t), 2, 2, 5, P(out), 4, P(dx), st))
    no("pool_bwd ld_dout < C", lib.pn2_pool_bwd_reduce_noact(P(x), 4, P(t), 8, P(x), 8, P(t), 2, 2, 5, P(out), P(red), st))
    no("pool_bwd ld_dout = 0 (a row-broadcast gradient)", lib.pn2_pool_bwd_reduce_noact(P(x), 0, P(t), 8, P(x), 8, P(t), 2, 2, 5, P(out), P(red), st))
    no("pool_bwd ldo < round4", lib.pn2_pool_bwd_reduce_noact(P(x), 5, P(t), 4, P(x), 8, P(t), 2, 2, 5, P(out), P(red), st))
    # pn2_conv1x1_fwd_gbias(X, ldx, W, ldw, bias, gbias, ldg, rows_per_group, Y, ldy, P, K, N, stats)
    no("gbias P % rows_per_group", lib.pn2_conv1x1_fwd_gbias(P(x), 4, P(t), 4, P(t), P(t), 8, 3, P(out), 8, 8, 4, 5, None, st))
    no("gbias ldg < N", lib.pn2_conv1x1_fwd_gbias(P(x), 4, P(t), 4, P(t), P(t), 4, 4, P(out), 8, 8, 4, 5, None, st))
    no("gbias ldy < round4", lib.pn2_conv1x1_fwd_gbias(P(x), 4, P(t), 4, P(t), P(t), 8, 4, P(out), 4, 8, 4, 5, None, st))
    # pn2_group_colsum(dZ, ldz, Y, ldy, coef, P, rows_per_group, C, s, lds, workspace)
    no("colsum lds < C", lib.pn2_group_colsum(P(x), 8, P(x), 8, P(t), 8, 4, 5, P(out), 4, P(ws), st))
    no("colsum P % rows_per_group", lib.pn2_group_colsum(P(x), 8, P(x), 8, P(t), 8, 3, 5, P(out), 8, P(ws), st))
    no("colsum G = 65536", lib.pn2_group_colsum(P(x), 4, P(x), 4, P(t), 65536, 1, 3, P(out), 4, P(ws), st))
    no("colsum workspace NULL", lib.pn2_group_colsum(P(x), 8, P(x), 8, P(t), 8, 4, 5, P(out), 8, None, st))
    # the multi-source GEMMs
    src = lambda n, K0=4: _lib.src_table([(P(x), 8, K0, None, 0)] * n)
    for nsrc in (0, 9):
        tb = src(max(nsrc, 1))
        no("fwd_multi nsrc = %d" % nsrc, lib.pn2_conv1x1_fwd_multi(tb, nsrc, P(t), 64, P(t), None, 8, 1, P(out), 8, 4, 5, None, st))
        no("wgrad_multi nsrc = %d" % nsrc, lib.pn2_conv1x1_wgrad_multi(P(x), 8, P(x), 8, P(t), tb, nsrc, P(dx), 64, None, 4, 5, st))
        ptrs, ld4, k4 = (ctypes.c_void_p * 9)(*[P(dx)] * 9), (ctypes.c_int * 9)(*[8] * 9), (ctypes.c_int * 9)(*[4] * 9)
        no("dgrad_multi nsrc = %d" % nsrc, lib.pn2_conv1x1_dgrad_multi(P(x), 8, P(x), 8, P(t), P(t), 64, ptrs, ld4, k4, nsrc, 4, 5, st))
    no("fwd_multi K % 4", lib.pn2_conv1x1_fwd_multi(src(2, 6), 2, P(t), 64, P(t), None, 8, 1, P(out), 8, 4, 5, None, st))
    no("wgrad_multi K % 4", lib.pn2_conv1x1_wgrad_multi(P(x), 8, P(x), 8, P(t), src(2, 6), 2, P(dx), 64, None, 4, 5, st))
    ptrs, ld4, k6 = (ctypes.c_void_p * 2)(P(dx), P(dx)), (ctypes.c_int * 2)(8, 8), (ctypes.c_int * 2)(4, 6)
    no("dgrad_multi K % 4", lib.pn2_conv1x1_dgrad_multi(P(x), 8, P(x), 8, P(t), P(t), 64, ptrs, ld4, k6, 2, 4, 5, st))
    no("fwd_multi P % rows_per_group", lib.pn2_conv1x1_fwd_multi(src(2), 2, P(t), 64, P(t), P(t), 8, 3, P(out), 8, 4, 5, None, st))
    # pn2_bn_bwd_reduce_noact_dense(dDense, ldd, dPool, ldp, arg, lda, Y, ldy, affine, G, K, C, dZ, ldz, red)
    no("dense dDense == dZ with ldd != ldz", lib.pn2_bn_bwd_reduce_noact_dense(P(out), 12, P(x), 8, P(t), 8, P(x), 8, P(t), 2, 2, 5, P(out), 8, P(red), st))
    no("dense lda % 4", lib.pn2_bn_bwd_reduce_noact_dense(P(x), 8, P(x), 8, P(t), 10, P(x), 8, P(t), 2, 2, 5, P(out), 8, P(red), st))
    no("dense ldz < round4", lib.pn2_bn_bwd_reduce_noact_dense(P(x), 8, P(x), 8, P(t), 8, P(x), 8, P(t), 2, 2, 5, P(out), 4, P(red), st))
    torch.cuda.synchronize()
    assert lib.pn2_point_transform_workspace_bytes(1, 2, 0) == 0 and lib.pn2_point_transform_workspace_bytes(1, 2, 129) == 0
    assert lib.pn2_group_colsum_workspace_bytes(8, 3, 5) == 0
    for name, b in (("out", out), ("dX", dx), ("dT", dt), ("workspace", ws), ("red", red)):
        assert bool((b.view(torch.int32) == K.SENTINEL).all()), "%s was written by a refused call" % name
    assert len(refused) == len(set(refused)) >= 40
