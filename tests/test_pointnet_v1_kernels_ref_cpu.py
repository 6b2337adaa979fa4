"""CPU: the statements, bounds, case tables and operand sets of tests/pointnet_v1_kernels_ref.py are themselves sound, and sharp.

(1) Each fp64 statement agrees with torch.autograd in fp64 on a small instance of the layer it serves, to 1e-12: bmm and its two
gradients, conv -> BatchNorm(train) -> max without a ReLU, the broadcast-concat layer, the dense head's bn5 consumed twice, and
the K-concatenated GEMMs.  (2) A float32 emulation of each kernel's arithmetic -- in the kernel's summation order where the
contract fixes it -- passes every check of tests/test_pointnet_v1_edges_gpu.py on every case of the tables (same seeds, same
shapes).  (3) Eleven mutants of the emulations each fail a check on EVERY case on which they change any bit of any output, and
each changes something on the cases its seam is named for.  Nothing here is fitted: a mutant that slipped through would be
answered by another case, not by a tighter bound.  (4) The seeds of the glue scenarios of tests/test_pointnet_v1_glue_gpu.py clear
their decision margins in fp64.
"""
import numpy as np
import pytest
import torch

import mlp_ref as R
import pointnet_v1_kernels_ref as K
import test_pointnet_v1_glue_gpu as GLUE

f32, f64 = np.float32, np.float64
T = torch.from_numpy


def n(t):
    return t.detach().numpy()


def close(got, want, what):
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), what


# ------------------------------------------------------------------------------------------------ (1) autograd

def test_transform_statements_agree_with_autograd():
    o = K.operands(11, "transform", B=2, N=7, k=5)
    B, N, k = 2, 7, 5
    x = T(o["X"][:, :k].astype(f64)).view(B, N, k).requires_grad_()
    t = T(o["T"].astype(f64)).requires_grad_()
    d = T(o["D"][:, :k].astype(f64)).view(B, N, k)
    out = torch.bmm(x, t)
    (out * d).sum().backward()
    close(K.point_transform(o["X"], o["ldx"], o["T"], B, N, k)[0], n(out).reshape(B * N, k), "out")
    dX, _, dT, _ = K.point_transform_bwd(o["D"], o["ldd"], o["X"], o["ldx"], o["T"], B, N, k)
    close(dX, n(x.grad).reshape(B * N, k), "dX")
    close(dT, n(t.grad), "dT")
    assert K.point_transform_workspace_bytes(3, 257, 5) == 3 * 2 * 25 * 4 and K.point_transform_workspace_bytes(3, 257, 129) == 0
    assert K.group_colsum_workspace_bytes(771, 257, 5) == 3 * 2 * 8 * 4 and K.group_colsum_workspace_bytes(770, 257, 5) == 0


def _bn_layer(g, P, C):
    gamma = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 1.0)
    gamma[1::3] *= -1.0
    return gamma.requires_grad_(), (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).requires_grad_()


def _blocks(Y, gamma, beta, P, eps=1e-5):
    blk = n(R.affine_block(Y.detach().sum(0), (Y.detach() ** 2).sum(0), P, gamma.detach(), beta.detach(), eps))
    return blk, K.block(*blk.astype(f32))            # (fp64 rows, and the float32 block layout the statements read)


def test_bn_max_statements_agree_with_autograd():
    """conv -> BatchNorm(train) -> max over K, no ReLU: bn_max, the routing of pool_bwd_reduce_noact and dY from its reductions."""
    g = torch.Generator().manual_seed(5)
    G, Kk, C = 4, 6, 7
    P = G * Kk
    Y = torch.randn(P, C, generator=g, dtype=torch.float64).requires_grad_()
    gamma, beta = _bn_layer(g, P, C)
    mean, var = Y.mean(0), Y.var(0, unbiased=False)
    z = (Y - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    out = z.view(G, Kk, C).max(1).values
    dOut = torch.randn(G, C, generator=g, dtype=torch.float64)
    (out * dOut).sum().backward()
    blk, _ = _blocks(Y, gamma, beta, P)
    zs = (n(Y) - blk[0]) * blk[1] + blk[2]
    arg = zs.reshape(G, Kk, C).argmax(1)
    close(zs.reshape(G, Kk, C).max(1), n(out), "out")
    # the reductions, stated on fp64 operands (the statement's float32 casts are the identity on float32 inputs)
    ys = np.take_along_axis(n(Y).reshape(G, Kk, C), arg[:, None, :], 1)[:, 0]
    r0, r1 = n(dOut).sum(0), (n(dOut) * (ys - blk[0]) * blk[3]).sum(0)
    D = np.zeros((G, Kk, C))
    np.put_along_axis(D, arg[:, None, :], n(dOut)[:, None, :], 1)
    coef = R.coef_block(T(r0), T(r1), P, gamma.detach(), T(blk[0]), T(blk[3]))
    close(n(R.dy_of(coef, T(D.reshape(P, C)), Y.detach())), n(Y.grad), "dY")
    close(r1, n(gamma.grad), "dgamma")
    close(r0, n(beta.grad), "dbeta")
    # and the float32 statements on float32 copies of the same operands agree with those to float32 accuracy of the operands
    o = dict(Y=K.padded(n(Y).astype(f32), 12), aff=K.block(*blk.astype(f32)))
    ro, ra = K.bn_max(o["Y"], 12, o["aff"], G, Kk, C)
    assert np.array_equal(ra, arg) and np.abs(ro - n(out)).max() < 1e-5
    dflat = np.concatenate([K.padded(n(dOut).astype(f32), C + 1, pad_to=C).reshape(-1), np.zeros(4, f32)])
    argb = np.zeros((G, 8), np.int32)
    argb[:, :C] = ra
    d, s0, _, s1, _ = K.pool_bwd_reduce_noact(dflat, C + 1, argb, 8, o["Y"], 12, o["aff"], G, Kk, C)
    assert np.array_equal(d, n(dOut).astype(f32)) and np.abs(s0 - r0).max() < 1e-5 and np.abs(s1 - r1).max() < 1e-4


def test_concat_layer_statements_agree_with_autograd():
    """relu(bn(conv(cat([g.repeat(N), pointfeat])))): conv1x1_fwd_gbias on the factorised form, group_colsum for the per-cloud part."""
    g = torch.Generator().manual_seed(6)
    B, N, cp, cg, co = 3, 5, 4, 8, 6
    P = B * N
    d64 = dict(generator=g, dtype=torch.float64)
    pf, gl = torch.randn(P, cp, **d64).requires_grad_(), torch.randn(B, cg, **d64).requires_grad_()
    W, b = (torch.randn(co, cg + cp, **d64) * 0.4).requires_grad_(), torch.randn(co, **d64).requires_grad_()
    gamma, beta = _bn_layer(g, P, co)
    cat = torch.cat([gl.repeat_interleave(N, 0), pf], 1)
    Y = cat @ W.t() + b
    Y.retain_grad()
    mean, var = Y.mean(0), Y.var(0, unbiased=False)
    z = torch.relu((Y - mean) / torch.sqrt(var + 1e-5) * gamma + beta)
    dOut = torch.randn(P, co, **d64)
    (z * dOut).sum().backward()
    gterm = n(gl) @ n(W)[:, :cg].T
    y_st = n(pf) @ n(W)[:, cg:].T + n(b) + np.repeat(gterm, N, 0)
    close(y_st, n(Y), "Y")
    # the float32 statement on float32 operands follows the same formula
    y32, _ = K.conv1x1_fwd_gbias(n(pf).astype(f32), cp, n(W)[:, cg:].astype(f32), n(b).astype(f32), gterm.astype(f32), co, N, P, cp, co)
    assert np.abs(y32 - y_st).max() < 1e-5
    blk, _ = _blocks(Y, gamma, beta, P)
    dZ = n(dOut) * (n(z) > 0)
    r0, r1 = dZ.sum(0), (dZ * (n(Y) - blk[0]) * blk[3]).sum(0)
    coef = n(R.coef_block(T(r0), T(r1), P, gamma.detach(), T(blk[0]), T(blk[3])))
    dY = coef[0] * dZ + coef[1] * (n(Y) - coef[3]) + coef[2]
    close(dY, n(Y.grad), "dY")
    s = dY.reshape(B, N, co).sum(1)
    close(s @ n(W)[:, :cg], n(gl.grad), "dg")
    close(s.T @ n(gl), n(W.grad)[:, :cg], "dW_g")
    close(dY.T @ n(pf), n(W.grad)[:, cg:], "dW_p")
    close(s.sum(0), n(b.grad), "db")
    s32, _ = K.group_colsum(K.padded(dZ.astype(f32), 8), 8, K.padded(n(Y).astype(f32), 12), 12, K.block(*coef.astype(f32)), P, N, co)
    assert np.abs(s32 - s).max() < 1e-5 * max(1.0, np.abs(s).max())


def test_dense_reduction_statement_agrees_with_autograd():
    """out5 = bn5(Y) consumed densely and by a max over each cloud: dZ = dDense + (k == arg) dPool, then dY from the reductions."""
    g = torch.Generator().manual_seed(7)
    G, Kk, C = 3, 5, 6
    P = G * Kk
    d64 = dict(generator=g, dtype=torch.float64)
    Y = torch.randn(P, C, **d64).requires_grad_()
    gamma, beta = _bn_layer(g, P, C)
    mean, var = Y.mean(0), Y.var(0, unbiased=False)
    out5 = (Y - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    dD, dP = torch.randn(P, C, **d64), torch.randn(G, C, **d64)
    ((out5 * dD).sum() + (out5.view(G, Kk, C).max(1).values * dP).sum()).backward()
    blk, _ = _blocks(Y, gamma, beta, P)
    arg = ((n(Y) - blk[0]) * blk[1] + blk[2]).reshape(G, Kk, C).argmax(1).astype(np.int32)
    o = dict(dD=n(dD).astype(f32), dP=n(dP).astype(f32), Y=n(Y).astype(f32))
    # stated in fp64 on the fp64 operands (the statement's own casts are applied to float32 buffers by the tests)
    hit = np.arange(Kk)[None, :, None] == arg[:, None, :]
    dZ = (n(dD).reshape(G, Kk, C) + np.where(hit, n(dP)[:, None, :], 0.0)).reshape(P, C)
    r0, r1 = dZ.sum(0), (dZ * (n(Y) - blk[0]) * blk[3]).sum(0)
    coef = R.coef_block(T(r0), T(r1), P, gamma.detach(), T(blk[0]), T(blk[3]))
    close(n(R.dy_of(coef, T(dZ), Y.detach())), n(Y.grad), "dY")
    close(r1, n(gamma.grad), "dgamma")
    close(r0, n(beta.grad), "dbeta")
    st = K.bn_bwd_reduce_noact_dense(o["dD"], C, o["dP"], C, arg, C, o["Y"], C, K.block(*blk.astype(f32)), G, Kk, C)
    assert np.abs(st[0] - dZ).max() < 1e-5 and np.abs(st[1] - r0).max() < 1e-4 and np.abs(st[3] - r1).max() < 1e-4


def test_multi_source_statements_agree_with_autograd():
    o = K.operands(13, "multi", P=9, N=5, mode="rpg1")
    P, N = 9, 5
    for s in o["srcs"]:
        if s[3] is not None:
            s[3][:K.round4(s[2])] = 0.0            # mean 0: the loader's float32 x - mean is exact, so fp64 autograd sees the same operand
    parts = []
    for X, ldx, Kk, aff, relu in o["srcs"]:
        x = T(X[:, :Kk].astype(f64)).requires_grad_()
        parts.append(x)
    acts = []
    for x, (X, ldx, Kk, aff, relu) in zip(parts, o["srcs"]):
        if aff is None:
            acts.append(x)
        else:
            a = T(aff.reshape(4, -1)[:, :Kk].astype(f64))
            v = (x - a[0]) * a[1] + a[2]
            acts.append(torch.relu(v) if relu else v)
    A = torch.cat(acts, 1)
    A.retain_grad()
    W = T(o["W"].astype(f64)).requires_grad_()
    b = T(o["bias"].astype(f64)).requires_grad_()
    Y = A @ W.t() + b + T(o["gbias"][:, :N].astype(f64))
    y_st, _ = K.conv1x1_fwd_multi(o["srcs"], o["W"], o["bias"], o["gbias"], o["ldg"], 1, P, N)
    close(y_st, n(Y), "Y")
    Yb = K.padded(n(Y).astype(f32), o["ldy"])
    dY, _ = K.dy_of(o["dZ"], o["ldz"], Yb, o["ldy"], o["coef"], P, N)
    (Y * T(dY)).sum().backward()
    dW, _, db, _ = K.conv1x1_wgrad_multi(o["dZ"], o["ldz"], Yb, o["ldy"], o["coef"], o["srcs"], P, N)
    close(dW, n(W.grad), "dW")
    close(db, n(b.grad), "dbias")
    k0 = 0
    for (dx, _), (X, ldx, Kk, aff, relu) in zip(K.conv1x1_dgrad_multi(o["dZ"], o["ldz"], Yb, o["ldy"], o["coef"], o["W"], [s[2] for s in o["srcs"]], P, N), o["srcs"]):
        close(dx, n(A.grad)[:, k0:k0 + Kk], "dX")              # (the gradient with respect to the ACTIVATED source: what the entry point hands back)
        k0 += Kk


# ------------------------------------------------------------------------------------------------ (2), (3) emulations and mutants

def _transform(c, m):
    _, seed, B, N, k = c
    o = K.operands(seed, "transform", B=B, N=N, k=k)
    out, dX = K.emulate_transform(o, False, m), K.emulate_transform(o, True, m)
    dT, ws = K.emulate_dt(o, m)
    return K.check_transform(o, out) + K.check_transform_bwd(o, dX, dT, ws, dT), (out, dX, dT, ws[K.point_transform_workspace_bytes(B, N, k) // 4:])


def _bn_max(c, m):
    _, seed, G, Kk, C, _ = c
    o = K.operands(seed, "bn_max", G=G, K=Kk, C=C)
    out, arg = K.emulate_bn_max(o, m)
    return K.check_bn_max(o, out, arg), (out, arg)


def _pool_bwd(c, m):
    _, seed, G, Kk, C, ldd, ldy, mode = c
    o = K.operands(seed, "pool_bwd", G=G, K=Kk, C=C, ld_dout=ldd, ldy=ldy, mode=mode)
    dzp, red = K.emulate_pool_bwd(o, m)
    return K.check_pool_bwd(o, dzp, red), (dzp, K.red_total(red, C))


def _gbias(c, m):
    _, seed, P, Kk, N, rpg, stats, ldg = c
    o = K.operands(seed, "gbias", P=P, K=Kk, N=N, rpg=rpg, ldg=ldg)
    Y, st = K.emulate_gbias(o, mutant=m)
    return K.check_gbias(o, Y, st if stats else None), (Y,) + ((K.red_total(st, N),) if stats else ())


def _colsum(c, m):
    _, seed, G, rpg, C, lds = c
    o = K.operands(seed, "colsum", G=G, rpg=rpg, C=C, lds=lds)
    s = K.emulate_colsum(o, m)
    return K.check_colsum(o, s, s), (s,)


def _dense(c, m):
    _, seed, G, Kk, C = c
    o = K.operands(seed, "dense", G=G, K=Kk, C=C)
    dZ, red = K.emulate_dense(o, mutant=m)
    dZa, reda = K.emulate_dense(o, mutant=m, alias=True)
    return K.check_dense(o, dZ, red) + K.check_dense(o, dZa, reda, alias=True), (dZ, K.red_total(red, C), dZa)


def _multi(c, m):
    _, seed, P, N, mode = c
    o = K.operands(seed, "multi", P=P, N=N, mode=mode)
    Y, st, dW, db, dX = K.emulate_multi(o)
    frame = np.zeros((N + 2, o["ldw"]), f32)
    frame[:N, o["off"]:o["off"] + o["Ktot"]] = dW
    return K.check_multi(o, Y, st if o["stats"] else None, frame, db, dX), (Y,)


FAMILIES = {
    "transform": (K.transform_cases, _transform, ("slab_last_row", "last_slab", "t_untransposed", "dt_store_past")),
    "bn_max": (K.bn_max_cases, _bn_max, ("last_k", "no_smaller_k", "idle_lane")),
    "pool_bwd": (K.pool_bwd_cases, _pool_bwd, ("pitch_for_width", "replica_missing")),
    "gbias": (K.gbias_cases, _gbias, ("gbias_late", "slab_last_row", "replica_missing")),
    "colsum": (K.colsum_cases, _colsum, ("slab_last_row", "last_slab")),
    "dense": (K.dense_cases, _dense, ("if_advance", "slab_last_row", "replica_missing")),
    "multi": (K.multi_cases, _multi, ()),
}
# the cases a mutant MUST change something on (its seam), by a substring of (or a predicate on) the case id; None: every case of
# the family.  (A 1 x 1 matrix is its own transpose; a tie, a fold rule or an idle lane matters on the (cloud, channel) entries whose
# planted pair or free maximum meets it, which a 65-channel case always has and a one-channel case may not.)
MUST = {("transform", "slab_last_row"): None, ("transform", "last_slab"): None, ("transform", "t_untransposed"): lambda i: " pad" in i and not i.startswith("k=1 "),
        ("transform", "dt_store_past"): " pad", ("bn_max", "last_k"): "C=65 K=65 ", ("bn_max", "no_smaller_k"): "C=65 K=65 ",
        ("bn_max", "idle_lane"): "C=65 K=2 ", ("pool_bwd", "pitch_for_width"): "G=3 ", ("pool_bwd", "replica_missing"): None,
        ("gbias", "gbias_late"): None, ("gbias", "slab_last_row"): None, ("gbias", "replica_missing"): "stats=1",
        ("colsum", "slab_last_row"): None, ("colsum", "last_slab"): None, ("dense", "if_advance"): "while-advance",
        ("dense", "slab_last_row"): None, ("dense", "replica_missing"): None}


def _same(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def test_mutant_table_is_complete():
    named = {m for _, _, ms in FAMILIES.values() for m in ms}
    assert named == set(K.MUTANTS) and set(MUST) == {(f, m) for f, (_, _, ms) in FAMILIES.items() for m in ms}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_emulation_stays_inside_the_bounds_and_mutants_do_not(family):
    cases, run, mutants = FAMILIES[family]
    changed = {m: 0 for m in mutants}
    for c in cases():
        bad, outs = run(c, None)
        assert not bad, (c[0], bad)
        for m in mutants:
            mbad, mouts = run(c, m)
            must = MUST[(family, m)]
            if _same(outs, mouts):
                assert must is not None and not (must(c[0]) if callable(must) else must in c[0]), "%s changes nothing on %r" % (m, c[0])
                continue
            changed[m] += 1
            assert mbad, "%s slips through on %r" % (m, c[0])
    assert all(changed.values()), changed


def test_case_tables_name_their_seams():
    ids = [c[0] for f in FAMILIES.values() for c in f[0]()]
    assert len(ids) == len(set(ids))
    for seam in ("k=60 q=15 1-idle one-lane", "k=33 q=9 4-idle dT-3-lanes 13-idle", "k=64 q=16 256-blocks", "k=61 q=16 256-blocks pad",
                 "k=65 q=17 1-idle 289-blocks 2-trips pad", "k=68 q=17 1-idle 289-blocks 2-trips", "k=20 q=5 1-idle", "k=100 q=25 6-idle",
                 "N=255 slab-1", "N=256 one-slab", "N=1 one-row", "N=3 rows<lanes", "N=600 three-slabs",
                 "G=65539 grid-stride", "arg=NULL", "K=65 lane-revisit", "K=2 62-idle-lanes", "G=4099 grid-stride",
                 "rpg=17 group-straddles-range", "rpg=1 group-per-row", "K=2 while-advance", "K=1 while-advance", "K=3 while-advance",
                 "K=63 straddle", "rows_per_group=1", "gbias=NULL stats", "rpg=257 slab+1"):
        assert any(seam in i for i in ids), seam
    # planted ties of bn_max: (k, k + 1), (k, k + 64), (0, K - 1) and (1, 64), each on channels of positive and of negative gamma,
    # and a channel of zero gamma wherever there are five channels
    seen = set()
    for _, seed, G, Kk, C, _ in K.bn_max_cases():
        o = K.operands(seed, "bn_max", G=G, K=Kk, C=C)
        for g, c in zip(*np.nonzero(o["plants"] >= 0)):
            k0, k1 = o["pairs"][o["plants"][g, c]]
            kind = "ends" if (k0, k1) == (0, Kk - 1) else "fold" if (k0, k1) == (1, 64) else k1 - k0
            if o["scale"][c] != 0:
                seen.add((kind, bool(o["scale"][c] > 0)))
        assert (o["scale"] == 0).any() or C < 5
    for kind in (1, 64, "ends", "fold"):
        assert (kind, True) in seen and (kind, False) in seen, (kind, seen)
    for _, seed, G, Kk, C in K.dense_cases(K.NOMINAL_CUS):
        P = G * Kk
        assert P > 128 and (P % 64 or Kk == 64)
        assert any((g * Kk) // 64 != ((g + 1) * Kk - 1) // 64 for g in range(G)) == (64 % Kk != 0)



# ------------------------------------------------------------------------------------------------ (4) decision margins of the glue scenarios

def test_glue_scenarios_clear_their_decision_margins():
    seen = set()
    for kind, shape, B, N, train, _, _ in GLUE.cases():
        key = (kind, shape, B, N, train)
        if key in seen:
            continue
        seen.add(key)
        S = GLUE.scenario(*key)
        kinds = [k for k, _ in S["margins"]]
        assert kinds == {"transform": [], "conv_bn_max": ["max"], "concat": ["relu"], "dense": ["max", "relu"]}[kind], key
        assert all(m > GLUE.MARGIN for _, m in S["margins"]), (key, S["seed"], S["margins"])
    assert {k[0] for k in seen} == set(GLUE.INPUTS) and {(k[2], k[3]) for k in seen} == set(GLUE.SHAPES)
