"""CPU: tests/corr_ransac_ref.py against independent statements -- the sampler against plane_ref's, the triad rule against a planted
transform, the Jacobi / Horn solve against numpy.linalg.eigh and SVD-Kabsch, the whole reference on planted pairs.

THE BOUND OF THE SOLVE.  An eigenvector of a symmetric matrix moves by at most |dN| / gap under a perturbation dN (Davis-Kahan),
and a backward-stable solver has |dN| = c * eps * ||N||_F: the top eigenvector is held to c * eps * ||N||_F / gap, gap = the
distance between eigh's two largest eigenvalues; the cases keep gap / ||N||_F >= 1e-3 (the smallest that occurs: 0.14).  MEASURED
here on the 200 cases below (a quarter each: generic, coplanar inliers, a flat set against its mirror image -- the case in which an
SVD without the determinant correction returns a reflection --, float32-valued points): the reference's eigenvector differs from
eigh's by at most 3.9 of these units, its transform from SVD-Kabsch's by at most 3.2 units of corr_ransac_ref.transform_tolerance.
c = corr_ransac_ref.C_HORN = 40, one order of magnitude above.  The off-diagonal norm of N falls to 5e-11, 1e-33, 2e-113, 0 of ||N||_F
after sweeps 4 .. 7: PN2_HORN_SWEEPS = 8 leaves three in hand."""
import numpy as np

import corr_ransac_ref as C
import plane_ref

worst = {"u": 0.0, "T": 0.0}


def solve_cases():
    rng = np.random.default_rng(0)
    for k in range(200):
        n = int(rng.integers(3, 400))
        p = rng.normal(size=(n, 3)) * rng.uniform(0.1, 5) + rng.normal(size=3) * rng.uniform(0, 20)
        kind = k % 4
        if kind == 1:
            p[:, 2] = 0.3 * p[:, 0] - 0.2 * p[:, 1] + 1.0            # coplanar inliers: S of rank 2
        R, t = C.rotation(rng.normal(size=3), rng.uniform(0, 180)), rng.normal(size=3) * 3
        q = p @ R.T + t + rng.normal(size=(n, 3)) * rng.choice([0, 1e-3, 5e-2])
        if kind == 2:                                                # reflection-prone: a flat set against its mirror image
            p[:, 2] *= 0.05
            q = (p * [1, 1, -1]) @ R.T + t + rng.normal(size=(n, 3)) * 1e-3
        if kind == 3:
            p, q = p.astype(np.float32).astype(np.float64), q.astype(np.float32).astype(np.float64)
        yield kind, p, q


def test_sampler_equals_plane_refs():
    for seed in (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1):
        for b in (0, 1, 65534):
            for n in (1, 3, 600, 2 ** 31 - 256):
                rows = plane_ref.sample_rows(seed, b, 300, n)
                for h in (0, 1, 7, 255, 299):
                    for j in range(3):
                        assert C.sample(seed, b, h, j, n) == plane_ref.sample(seed, b, h, j, n) == rows[h, j] < n


def test_triad_returns_the_planted_transform():
    rng = np.random.default_rng(3)
    for _ in range(50):
        R, t = C.rotation(rng.normal(size=3), rng.uniform(0, 180)), rng.normal(size=3) * 4
        p = rng.normal(size=(1, 3, 3)) * 2
        q = p @ R.T + t
        T, lwp, lwq = C.triad(p, q)
        assert lwp[0] > 0 and lwq[0] > 0
        want = np.concatenate([R, t[:, None]], 1).reshape(12)
        assert np.abs(T[0] - want).max() <= 1e-12 * (1 + np.abs(p).max() / min(lwp[0], lwq[0]))
        Rm = T[0].reshape(3, 4)[:, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-14 and np.linalg.det(Rm) > 0


def test_triad_of_a_degenerate_triple_is_invalid():
    src = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 0]])[None]       # rows 0, 1, 2 collinear; row 4 repeats row 0
    tgt = src.copy()
    ps = np.arange(5)[None]
    for h in range(64):
        T, ok, rows = C.hypotheses(src[0], tgt[0], ps[0], ps[0], 5, 0, 0, 64, 0.0)
    r = {tuple(sorted(x)) for x in rows[ok]}
    assert ok.any() and (0, 1, 2) not in r and all(not ({0, 4} <= set(x)) and len(set(x)) == 3 for x in r)
    assert np.isnan(T[~ok]).all() and np.isfinite(T[ok]).all()


def test_horn_against_eigh_and_kabsch():
    seen = set()
    for kind, p, q in solve_cases():
        S, AS = C.refit_sums(p, q, np.zeros(len(p)))
        scale, rel, v = C.horn_bound(S)
        assert rel >= 1e-3
        A, n = C.horn_matrix(S)
        diag, V, off = C.jacobi4(A)
        assert off[-1] <= 2.0 ** -52 * np.linalg.norm(A)
        u = C.largest(diag, V)
        u = u / np.linalg.norm(u)
        v = v if v @ u > 0 else -v
        worst["u"] = max(worst["u"], float(np.linalg.norm(u - v) / scale))
        assert np.linalg.norm(u - v) <= C.C_HORN * scale
        T, deg = C.horn(S)
        assert not deg
        Rm = T.reshape(3, 4)[:, :3]
        assert np.linalg.det(Rm) > 0 and np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-14          # a rotation, never a reflection
        tol = C.transform_tolerance(S, AS)
        err = np.abs(T - C.kabsch(p, q))
        worst["T"] = max(worst["T"], float((err / tol).max() * C.C_HORN))
        assert (err <= tol).all()
        seen.add(kind)
    print("worst eigenvector error %.2f units, worst |T - kabsch| %.2f units (c = %g)" % (worst["u"], worst["T"], C.C_HORN))
    assert seen == {0, 1, 2, 3}


def test_horn_degenerate():
    S = np.zeros(C.SUMS)
    assert C.horn(S) == (None, True)
    p = np.float64([[0, 0, 0], [1, 0, 0]])
    S, _ = C.refit_sums(p, p, np.zeros(2))
    assert C.horn(S)[1]                                              # two inliers


def test_reference_recovers_planted_pairs():
    rng = np.random.default_rng(5)
    N = 200
    src = rng.uniform(-1, 1, (1, N, 3)).astype(np.float32)
    R, t = C.rotation((1, 2, 3), 140.0), np.array([0.5, -0.25, 1.0])
    tgt = (src[0].astype(np.float64) @ R.T + t).astype(np.float32)[None]
    ps = np.arange(N)[None]
    pt = ps.copy()
    pt[0, N // 2:] = rng.integers(0, N, N - N // 2)                  # half the pairs are random
    out = C.ransac(src, tgt, ps, pt, 0.01, 256)
    assert out["status"][0] == 0 and out["err"] == 0 and out["best_count"][0] >= N // 2
    r = C.refit(src[0], tgt[0], ps[0], pt[0], N, out["T"][0], 0.01)
    assert not r["degenerate"] and r["count"] >= N // 2
    assert np.abs(C.apply(r["T"], src[0].astype(np.float64)) - tgt[0]).max() <= 1e-6
    out0 = C.ransac(src, tgt, ps, pt, 0.01, 256, count=[2])
    assert out0["status"][0] == C.NONE and out0["err"] == C.ERR_NONE and (out0["T"][0] == C.IDENTITY).all() and (out0["hyp_count"] == -1).all()
