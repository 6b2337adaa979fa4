"""CPU: the statements, bounds and operand sets of tests/bn_pool_ref.py are themselves sound, and sharp.

(1) The fp64 statements agree with torch.autograd in fp64 on a small conv -> BatchNorm(train) -> ReLU -> max over K and on its
dense form, to 1e-12.  (2) A float32 emulation of the kernels' two x-hat formulas, with the branch rule as include/pn2.h states
it, stays inside the a-priori bounds on every operand set tests/test_bn_pool_gpu.py uses (same seeds, same shapes, drawn on
the CPU).  (3) Seven mutants of that emulation -- the last group dropped, a group counted twice, row arg + 1 gathered, the
`out` branch without its division by gamma, the mask taken as out >= 0, "last k wins" on ties, row 0 not forced for a zero
scale -- violate a bound or an exact comparison on EVERY case they could affect: what the GPU test asserts would catch a
subtly wrong kernel.  Nothing here is fitted: a mutant that slipped through would be answered by other operands, not by a
tighter bound.
"""
import numpy as np
import pytest
import torch

import bn_pool_ref as B
import mlp_ref as R

NOMINAL_CUS = 256                    # the case tables depend on the device's compute units; an MI355X has 256


# ------------------------------------------------------------------------------------------------ the checks of the GPU test

def reduce_ok(c, st, dz, red0, red1):
    """What tests/test_bn_pool_gpu.py asserts of a reduction: dZp bit-equal, red0 exact, red1 within its bound."""
    return (np.array_equal(dz, st["dZp"]) and np.array_equal(red0, st["red0"]) and bool((np.abs(red0 - st["red0"]) <= st["b0"]).all())
            and bool((np.abs(red1 - st["red1"]) <= st["b1"]).all()))


def _reduce_sets():
    out = []
    for seed, G, K, C, ci in B.reduce_cases():
        c = B.reduce_case(seed, G, K, C, C_in=ci)
        out.append(("pool %d" % seed, c, False))
        out.append(("rec %d" % seed, c, True))
    for seed, P, C in B.dense_cases():
        out.append(("dense %d" % seed, B.reduce_case(seed, P, 1, C, dense=True), False))
    return out


REDUCE_SETS = _reduce_sets()


# ------------------------------------------------------------------------------------------------ (1) autograd

@pytest.mark.parametrize("K", [1, 5])
def test_statements_agree_with_autograd(K):
    """conv -> BatchNorm (training) -> ReLU -> max over K (K = 1: the dense form) in fp64 torch: the pooled output, the routing
    of dZp, and dY / dgamma / dbeta built from the two reductions through coef_block / dy_of."""
    g = torch.Generator().manual_seed(3 + K)
    G, Ci, C, eps = 7, 6, 11, 1e-5
    P = G * K
    X = torch.randn(P, Ci, generator=g, dtype=torch.float64)
    W = torch.randn(C, Ci, generator=g, dtype=torch.float64) * 0.5
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    gamma = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 1.0).requires_grad_()
    gamma.data[1::3] *= -1.0
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).requires_grad_()
    Y = (X @ W.t() + b).requires_grad_()
    mean, var = Y.mean(0), Y.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    act = torch.relu((Y - mean) * invstd * gamma + beta)
    out = act.view(G, K, C).max(1).values
    dOut = torch.randn(G, C, generator=g, dtype=torch.float64)
    (out * dOut).sum().backward()

    n = lambda t: t.detach().numpy()
    blk = n(R.affine_block(Y.detach().sum(0), (Y.detach() ** 2).sum(0), P, gamma.detach(), beta.detach(), eps))
    o_ref, arg = B.pool_fwd(n(Y).reshape(G, K, C), blk[0], blk[1], blk[2])
    assert np.abs(o_ref - n(out)).max() <= 1e-12 * np.abs(n(out)).max()
    ystar = np.take_along_axis(n(Y).reshape(G, K, C), arg[:, None, :].astype(np.int64), 1)[:, 0]
    c = dict(G=G, K=K, C=C, mean=blk[0], scale=blk[1], beta=blk[2], invstd=blk[3], out=o_ref, dOut=n(dOut), ystar=ystar)
    st = B.reduce_statement(c)
    assert np.array_equal(st["dZp"], np.where(n(out) > 0, n(dOut), 0.0))
    D = np.zeros((G, K, C))
    np.put_along_axis(D, arg[:, None, :].astype(np.int64), st["dZp"][:, None, :], 1)
    T = torch.from_numpy
    coef = R.coef_block(T(st["red0"]), T(st["red1"]), P, gamma.detach(), T(blk[0]), T(blk[3]))
    dY = n(R.dy_of(coef, T(D.reshape(P, C)), Y.detach()))
    for got, want, what in ((dY, n(Y.grad), "dY"), (st["red1"], n(gamma.grad), "dgamma"), (st["red0"], n(beta.grad), "dbeta")):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what


# ------------------------------------------------------------------------------------------------ (2) the emulation is inside

def test_operand_sets_cover_what_they_claim():
    kinds, last_row, branches = set(), 0, set()
    for name, c, rec in REDUCE_SETS:
        if rec:
            continue
        G, K, C = c["G"], c["K"], c["C"]
        frac = float(((c["out"] <= 0) & (c["dOut"] != 0)).mean())
        assert frac >= 0.2 or G * C < 5, (name, frac)               # (one entry cannot be a fifth masked and live at once)
        kinds |= set(c["kind"].tolist())
        branches |= set(B.from_out(c)[0].tolist())
        last_row += int((c["Y"][-1] != B.POISON).any() and K > 1)
        fo = B.from_out(c)[0]
        assert bool(fo[np.isin(c["kind"], (0, 3, 5))].all()) and not bool(fo[np.isin(c["kind"], (2, 4, 6))].any()), name
    assert kinds == set(range(8)) and branches == {True, False} and last_row >= 10


@pytest.mark.parametrize("name,c,rec", REDUCE_SETS, ids=[s[0].replace(" ", "-") for s in REDUCE_SETS])
def test_emulation_stays_inside_the_bounds_and_mutants_do_not(name, c, rec):
    st = B.reduce_statement(c, rec=rec)
    dz, red0, red1 = B.emulate_reduce(c, rec=rec)
    assert np.array_equal(dz, st["dZp"]) and np.array_equal(red0, st["red0"])
    worst = float((np.abs(red1 - st["red1"]) / np.maximum(st["b1"], 1e-300)).max())
    assert worst <= 1.0, worst
    live = st["live"]
    fo = st["branch"]
    gam = c["scale"].astype(np.float64) / c["invstd"].astype(np.float64)
    could = {1: True,
             2: bool(live[0].any()),
             3: not rec and bool(live[:, ~fo].any()),
             4: not rec and bool(live[:, fo & (np.abs(np.abs(gam) - 1.0) > 1e-3)].any()),
             5: bool((c["out"] == 0).any())}
    for m, affected in could.items():
        ok = reduce_ok(c, st, *B.emulate_reduce(c, mutant=m, rec=rec))
        assert not (affected and ok), "mutant %d passes on %s" % (m, name)
        assert affected or ok, "mutant %d is rejected on %s although it cannot affect it" % (m, name)


def test_every_reduce_mutant_is_exercised():
    n = {m: 0 for m in (2, 3, 4)}
    for name, c, rec in REDUCE_SETS:
        st = B.reduce_statement(c, rec=rec)
        n[2] += bool(st["live"][0].any())
        n[3] += (not rec) and bool(st["live"][:, ~st["branch"]].any())
        n[4] += (not rec) and bool(st["live"][:, st["branch"]].any())
    assert min(n.values()) >= 20, n


# ------------------------------------------------------------------------------------------------ (3) forward: ties, zero scale

LATTICE = B.relu_max_cases(NOMINAL_CUS)


@pytest.mark.parametrize("form,seed,G,K,C", LATTICE, ids=["%s-%d" % (c[0], c[1]) for c in LATTICE])
def test_lattice_cases_are_exact_hold_their_plants_and_reject_last_k_wins(form, seed, G, K, C):
    assert B.relu_max_form(NOMINAL_CUS, G, K, C)[0] == form
    c = B.lattice_case(seed, G, K, C)
    out, arg = B.emulate_relu_max(c)
    assert np.array_equal(out, c["out"]) and np.array_equal(arg, c["arg"])
    p, nz = c["plants"], c["scale"] != 0
    rpw = B.lane_geometry(C)[1]
    assert ("tie_lane" in p) == (K > 1 and rpw < K) and ("tie_quarter" in p) == (K >= 32)
    if "tie_lane" in p:
        g, k0, k1 = p["tie_lane"]
        assert k1 == k0 + rpw and bool((c["arg"][g, nz] <= k0).all()) and np.array_equal(c["Y"][g, k0], c["Y"][g, k1])
    if "tie_quarter" in p:
        g, k0, k1 = p["tie_quarter"]
        kq = (K + 3) >> 2
        assert k0 // kq != k1 // kq and bool((c["arg"][g, nz] <= k0).all())
    if K > 1 and G >= 4:
        assert bool((c["arg"][p["all_equal"]] == 0).all())
        g = p["all_nonpositive"]
        assert bool((c["out"][g, nz] == 0).all()) and bool((c["arg"][g, nz] == 0).all())
    assert bool((c["arg"][:, ~nz] == 0).all())
    if K > 1:                                                        # mutant 6: every case with more than one row has a planted tie
        out6, arg6 = B.emulate_relu_max(c, mutant=6)
        assert np.array_equal(out6, c["out"]) and not np.array_equal(arg6, c["arg"])


@pytest.mark.parametrize("relu", [True, False])
def test_negative_scale_picks_the_smallest_y(relu):
    c = B.lattice_case(77, 6, 40, 20, relu=relu)
    neg = c["scale"] < 0
    ysel = np.take_along_axis(c["Y"], c["arg"][:, None, :].astype(np.int64), 1)[:, 0]
    win = c["out"] > 0 if relu else np.ones_like(c["out"], bool)
    assert bool(neg.any()) and bool((ysel[:, neg] == c["Y"].min(1)[:, neg])[win[:, neg]].all())


@pytest.mark.parametrize("seed,G,C", B.select_cases(NOMINAL_CUS))
def test_record_cases_reject_a_zero_scale_that_keeps_its_record(seed, G, C):
    c = B.record_case(seed, G, 64, C)
    out, arg = B.emulate_pool_select(c)
    assert np.array_equal(out, c["out"]) and np.array_equal(arg, c["arg"])
    assert bool((c["scale"] == 0).any()) and bool((c["scale"] < 0).any())
    out7, arg7 = B.emulate_pool_select(c, mutant=7)
    assert not np.array_equal(arg7, c["arg"])


def test_cancelling_channel_and_ulp_measure():
    s = B.stats_case(9, 1000, 5)
    cc = s["cancel"]
    assert s["s2"][cc] / 1000 - (s["s1"][cc] / 1000) ** 2 < 0
    blk = R.affine_block(torch.from_numpy(s["s1"]), torch.from_numpy(s["s2"]), 1000, torch.from_numpy(s["gamma"]), torch.from_numpy(s["beta"]), 1e-5)
    assert abs(float(blk[3, cc]) - 1e-5 ** -0.5) < 1e-9
    x = np.float32(1.5)
    assert B.ulps(np.nextafter(x, np.float32(2)), np.float64(1.5)) == 1.0 and B.ulps(x, np.float64(1.5)) == 0.0
