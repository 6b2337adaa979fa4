"""CPU: the fp64 statements, the derived bound and the generators of tests/scatter_ref.py are checked on their own, so
that a HIP kernel is only ever held to a reference and a tolerance that were shown valid without it."""
import numpy as np
import pytest
import torch

import scatter_ref as R
from conftest import golden
from oracle import geometry as G


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_scatter_sum_equals_a_naive_double_loop():
    rng = np.random.default_rng(0)
    B, M, T, D = 2, 37, 5, 3
    idx = rng.integers(-1, T + 2, (B, M))                       # -1, T and T + 1 are out of range: dropped
    terms = rng.normal(size=(B, M, D))
    out, n, A = R.scatter_sum(torch.from_numpy(idx), torch.from_numpy(terms), T)
    ref, rn, rA = np.zeros((B, T, D)), np.zeros((B, T)), np.zeros((B, T, D))
    for b in range(B):
        for m in range(M):
            if 0 <= idx[b, m] < T:
                ref[b, idx[b, m]] += terms[b, m]
                rA[b, idx[b, m]] += np.abs(terms[b, m])
                rn[b, idx[b, m]] += 1
    assert np.allclose(out.numpy(), ref, rtol=0, atol=1e-13) and np.array_equal(n.numpy(), rn)
    assert np.allclose(A.numpy(), rA, rtol=0, atol=1e-13)


def test_backward_statements_equal_naive_loops():
    rng = np.random.default_rng(1)
    B, N, S, K, D, C = 2, 6, 4, 3, 5, 6
    # interpolation
    idx = torch.from_numpy(rng.integers(0, S, (B, N, 3)))
    g, w = torch.from_numpy(rng.normal(size=(B, N, D + 3))), torch.from_numpy(rng.uniform(size=(B, N, 3)))
    out, n, _ = R.interp_bwd(g, 2, D, idx, w, S)
    ref = np.zeros((B, S, D))
    for b in range(B):
        for i in range(N):
            for k in range(3):
                ref[b, idx[b, i, k]] += w[b, i, k].item() * g[b, i, 2:2 + D].numpy()
    assert np.allclose(out.numpy(), ref, rtol=0, atol=1e-13) and float(n.sum()) == B * N * 3
    # grouping (both column orders, idx None, an index equal to N dropped) and the row gather
    gidx = torch.from_numpy(rng.integers(0, N + 1, (B, S, K)))
    rows = torch.from_numpy(rng.normal(size=(B * S * K, D + 3)))
    for xyz_first in (0, 1):
        out, n, _ = R.group_bwd(rows, gidx, B, N, S, K, D, xyz_first)
        ref = np.zeros((B, N, D))
        for p in range(B * S * K):
            j = int(gidx.reshape(-1)[p])
            if j < N:
                ref[p // (S * K), j] += rows[p, 3 * xyz_first:3 * xyz_first + D].numpy()
        assert np.allclose(out.numpy(), ref, rtol=0, atol=1e-13)
        assert float(n.sum()) == float((gidx < N).sum())
    full = torch.from_numpy(rng.normal(size=(B * S * N, D + 3)))            # idx == NULL: K == N, member k of every group
    out, _, _ = R.group_bwd(full, None, B, N, S, N, D, 0)
    assert np.allclose(out.numpy(), full[:, :D].reshape(B, S, N, D).sum(1).numpy(), rtol=0, atol=1e-13)
    out, _, _ = R.gather_rows_bwd(rows[:B * 7, :D].reshape(B, 7, D), torch.from_numpy(rng.integers(0, N, (B, 7))), N)
    assert abs(float(out.sum()) - float(rows[:B * 7, :D].sum())) < 1e-12
    # factorised first layer, forward and backward
    xyz, ctr = torch.from_numpy(rng.normal(size=(B, N, 3))), torch.from_numpy(rng.normal(size=(B, S, 3)))
    Zf, Wx = torch.from_numpy(rng.normal(size=(B * N, C))), torch.from_numpy(rng.normal(size=(C, 3)))
    aidx = torch.from_numpy(rng.integers(0, N, (B, S, K)))
    Y, mag, s0, s1 = R.group_affine_fwd(Zf, xyz, ctr, aidx, Wx)
    dZ = torch.from_numpy(rng.normal(size=(B * S * K, C)))
    coef = tuple(torch.from_numpy(rng.normal(size=C)) for _ in range(4))
    dY, Gs, n, A, dWx, _ = R.group_affine_bwd(dZ, Y, coef, xyz, ctr, aidx)
    rG, rW = np.zeros((B, N, C)), np.zeros((C, 3))
    for b in range(B):
        for s in range(S):
            for k in range(K):
                p, j = (b * S + s) * K + k, int(aidx[b, s, k])
                d = (xyz[b, j] - ctr[b, s]).numpy()
                y = Zf[b * N + j].numpy() + Wx.numpy() @ d
                assert np.allclose(Y[p].numpy(), y, rtol=0, atol=1e-12)
                assert (mag[p].numpy() >= np.abs(y) - 1e-12).all()
                dy = coef[0].numpy() * dZ[p].numpy() + coef[1].numpy() * (y - coef[3].numpy()) + coef[2].numpy()
                rG[b, j] += dy
                rW += np.outer(dy, d)
    assert np.allclose(Gs.numpy(), rG, rtol=0, atol=1e-12) and np.allclose(dWx.numpy(), rW, rtol=0, atol=1e-12)
    assert np.allclose(s0.numpy(), Y.numpy().sum(0)) and np.allclose(s1.numpy(), (Y.numpy() ** 2).sum(0))
    assert (A.numpy() >= np.abs(Gs.numpy()) - 1e-12).all() and float(n.sum()) == B * S * K


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 300, 5000, 196608])
def test_float32_sums_in_three_orders_stay_inside_the_bound(n):
    """The bound is valid for the reference alone: w * g terms (one rounding each) and dY terms (three roundings each)
    of the generators the GPU tests use, summed in float32 sequentially, reversed and pairwise."""
    D = 4 if n > 5000 else 16
    N = -(-n // 3)
    g, w = R.random_interp_data(1, N, D, n)
    t64 = (w.double().unsqueeze(3) * g.double().unsqueeze(2)).reshape(3 * N, D)[:n]
    t32 = (w.unsqueeze(3) * g.unsqueeze(2)).reshape(3 * N, D)[:n].numpy()                   # float32 products
    dZ, Y, (c0, q1, q0, mu), _, _ = R.random_affine_data(1, 1, 1, n, D, n + 1)
    d64 = c0.double() * dZ.double() + q1.double() * (Y.double() - mu.double()) + q0.double()
    a64 = (c0.double() * dZ.double()).abs() + (q1.double() * (Y.double() - mu.double())).abs() + q0.double().abs()
    d32 = (c0 * dZ + (q1 * (Y - mu) + q0)).numpy()                                          # float32, separately rounded
    worst = 0.0
    for t32_, ref, A in ((t32, t64.sum(0), t64.abs().sum(0)), (d32, d64.sum(0), a64.sum(0))):
        b = R.bound(n, A).numpy()
        for s in R.f32_sums_three_orders(t32_):
            err = np.abs(s.astype(np.float64) - ref.numpy())
            assert (err <= b).all(), (n, float((err / b).max()))
            worst = max(worst, float((err / b).max()))
    print("n = %d: worst error / bound = %.3f" % (n, worst))


@pytest.mark.parametrize("n", [1, 5, 64, 4097, 196608])
def test_exactly_summable_data_sums_bit_equal_in_every_order(n):
    D = 4
    N = -(-n // 3)
    g, w = R.exact_interp_data(1, N, D, n)
    t64 = (w.double().unsqueeze(3) * g.double().unsqueeze(2)).reshape(3 * N, D)[:n]
    R.assert_exactly_summable(t64.abs().sum(0), R.EXACT_INTERP_UNIT)
    assert bool(((t64 / R.EXACT_INTERP_UNIT) == (t64 / R.EXACT_INTERP_UNIT).round()).all())
    for s in R.f32_sums_three_orders(t64.float().numpy()):
        assert (bits(s) == bits(t64.sum(0).float().numpy())).all()
    dZ, Y, (c0, q1, q0, mu), xyz, ctr = R.exact_affine_data(1, 7, 1, n, D, n)
    d32 = c0 * dZ + (q1 * (Y - mu) + q0)
    d64 = c0.double() * dZ.double() + q1.double() * (Y.double() - mu.double()) + q0.double()
    assert bool((d32.double() == d64).all())                      # every term is exact in float32
    assert bool(((d64 / R.EXACT_AFFINE_UNIT_G) == (d64 / R.EXACT_AFFINE_UNIT_G).round()).all())
    a64 = (c0 * dZ).abs().double() + (q1 * (Y - mu)).abs().double() + q0.abs().double()
    assert float(a64.max()) <= 1.375
    R.assert_exactly_summable(a64.sum(0), R.EXACT_AFFINE_UNIT_G)
    for s in R.f32_sums_three_orders(d32.numpy()):
        assert (bits(s) == bits(d64.sum(0).float().numpy())).all()
    idx = R.random_index(1, n, 7, n).view(1, 1, n)
    _, _, _, _, dWx, AW = R.group_affine_bwd(dZ, Y, (c0, q1, q0, mu), xyz, ctr, idx)
    R.assert_exactly_summable(AW, R.EXACT_AFFINE_UNIT_DWX)
    assert bool(((dWx / R.EXACT_AFFINE_UNIT_DWX) == (dWx / R.EXACT_AFFINE_UNIT_DWX).round()).all())


def test_group_affine_forward_float32_evaluation_inside_its_bound():
    """Y = fma(Wx2, d2, fma(Wx1, d1, fma(Wx0, d0, z))) with d = fl(xyz - centre): one rounded difference and three fmas
    (evaluated here with each fma as an exact fp64 product-sum rounded once to float32) stay within 5 u mag."""
    B, N, S, K, C = 2, 50, 8, 16, 12
    g = torch.Generator().manual_seed(3)
    xyz, ctr = torch.rand(B, N, 3, generator=g) * 2 - 1, torch.rand(B, S, 3, generator=g) * 2 - 1
    Zf, Wx = torch.randn(B * N, C, generator=g), torch.randn(C, 3, generator=g) * 0.3
    idx = R.random_index(B, S * K, N, 4).view(B, S, K)
    Y, mag, _, _ = R.group_affine_fwd(Zf, xyz, ctr, idx, Wx)
    rows = (idx + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    d = (xyz.reshape(-1, 3)[rows].view(B, S, K, 3) - ctr.unsqueeze(2)).reshape(-1, 3)          # float32 difference
    y = Zf[rows]
    for a in range(3):          # |product| < 2^-1 * 2^2: 48 significant bits, the fp64 sum below rounds once more at 2^-53
        y = (Wx[:, a].double() * d[:, a:a + 1].double() + y.double()).float()
    err = (y.double() - Y).abs()
    assert bool((err <= 5 * R.U32 * mag).all()), float((err / (R.U32 * mag)).max())


def test_interp_fwd_is_the_separately_rounded_statement():
    """Bit-equal to the oracle's C restatement (un-fused multiplies and adds in the reference's order) on the recorded
    cases, and within the fixture's own 2e-6 of its recorded `interp` (recorded from a framework sum over the three
    neighbours, whose order the fixture does not fix -- tests/test_oracle_golden.py holds the oracle to the same)."""
    g = golden("g4_interp.npz")
    for tag in "abc":
        idx, dist = G.three_nn(g[tag + "/xyz1"], g[tag + "/xyz2"])
        w = G.three_weights(dist)
        mine = R.interp_fwd(torch.from_numpy(g[tag + "/points2"]), torch.from_numpy(idx), torch.from_numpy(w)).numpy()
        assert (bits(mine) == bits(G.three_interpolate(g[tag + "/points2"], idx, w))).all(), tag
        assert np.abs(mine - g[tag + "/interp"]).max() <= 2e-6


def test_index_generators_do_what_they_claim():
    M = 4 * 341 - 1                                  # 1363: neither a multiple of 4 nor of a chunk
    seen = set()
    for name, idx, T in R.constructed_cases(M, 11):
        assert idx.shape == (3, M) and idx.dtype == torch.int64
        assert int(idx.min()) >= 0 and int(idx.max()) < T
        assert not torch.equal(idx[0], idx[1])                            # different per cloud
        lens = R.segment_lengths(idx, T)
        assert (lens.sum(1) == M).all()
        seen.add(name)
        if name.startswith("len"):
            length = int(name[3:])
            for b in range(3):
                nz = lens[b][lens[b] > 0]
                assert (nz[:-1] == length).all() and nz[-1] == (M % length or length)
                assert (lens[b] == 0).sum() == 7                          # empty targets between the owners
        elif name == "one_owner":
            assert ((lens > 0).sum(1) == 1).all() and lens.max() == M
        elif name == "three_targets":
            assert T == 3 and (lens > max(R.CHUNKS)).all()                # each longer than the longest chunk
        else:
            assert ((lens == 0).sum(1) > 2 * M).all()
    assert seen == {"len%d" % n for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)} | {"one_owner", "three_targets", "mostly_empty"}
    base = R.segments_index(2, 1000, 40, 32, 5)
    dropped = R.with_dropped(base, 40, 6)
    out = (dropped < 0) | (dropped >= 40)
    assert (out.sum(1) == 100).all() and set(dropped[out].tolist()) == {-1, 45}
    assert torch.equal(dropped[~out], base[~out])
    assert (R.segment_lengths(dropped, 40).sum(1) == 900).all()
