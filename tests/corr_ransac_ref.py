"""The rule of include/pn2.h ("correspondence RANSAC") in numpy: what pn2_corr_ransac and pn2_corr_refit must write.

Every floating-point term is the fp64 statement of the header, one rounding per operation (numpy never fuses).  The sampler is the
header's integer function on Python integers (``sample``; tests/test_corr_ransac_cpu.py compares it with plane_ref's) and on uint64
arrays (plane_ref.sample_rows).  ``refit_sums`` adds the seventeen terms with numpy's sum -- the device adds the SAME terms in
another order, so ``abs_sums`` is what a test scales its bound by -- and ``horn`` is the part after the sums, usable on the DEVICE's
own sums.  ``jacobi4`` restates csrc/sym_eig4.h.  ``bump_scene`` is the end-to-end test's scene."""
import numpy as np

import plane_ref

NONE, DEGENERATE = 1, 2
ERR_PAIR, ERR_NONFINITE, ERR_NONE = 1, 2, 4
SUMS = 17
SWEEPS = 8                       # PN2_HORN_SWEEPS
MASK = (1 << 64) - 1
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
IDENTITY = np.eye(3, 4).reshape(12)


def sample(seed, b, h, j, n):
    """csrc/ransac_sample.h on Python integers: row j of hypothesis h of cloud b among n rows."""
    x = (seed * 0x9E3779B97F4A7C15 + ((b << 40) | (h << 8) | j)) & MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return ((x >> 32) * n) >> 32


def _len(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def frame(a0, a1, a2):
    """The header's FRAME of [H,3] fp64 triples -> (E [H,3,3] with E[:, k] = e_(k+1), c [H,3], |w| [H])."""
    u = a1 - a0
    e1 = u / _len(u)[..., None]
    w = _cross(e1, a2 - a0)
    lw = _len(w)
    e3 = w / lw[..., None]
    e2 = _cross(e3, e1)
    return np.stack([e1, e2, e3], -2), ((a0 + a1) + a2) / 3.0, lw


def triad(p, q):
    """p, q [H,3,3] fp64 (triple, point, axis) -> (T [H,12], |w| of both sides)."""
    E, c, lwp = frame(p[:, 0], p[:, 1], p[:, 2])
    F, cq, lwq = frame(q[:, 0], q[:, 1], q[:, 2])
    T = np.zeros((len(p), 3, 4))
    for a in range(3):
        for k in range(3):
            T[:, a, k] = (F[:, 0, a] * E[:, 0, k] + F[:, 1, a] * E[:, 1, k]) + F[:, 2, a] * E[:, 2, k]
        T[:, a, 3] = cq[:, a] - ((T[:, a, 0] * c[:, 0] + T[:, a, 1] * c[:, 1]) + T[:, a, 2] * c[:, 2])
    return T.reshape(-1, 12), lwp, lwq


def hypotheses(src_b, tgt_b, ps, pt, n, seed, b, H, edge_ratio):
    """-> (T [H,12] fp64 with NaN rows for invalid hypotheses, valid bool [H], rows [H,3])."""
    N, M = len(src_b), len(tgt_b)
    rows = plane_ref.sample_rows(seed, b, H, n)
    T = np.full((H, 12), np.nan)
    if n < 3:
        return T, np.zeros(H, bool), rows
    s, t = ps[rows], pt[rows]
    ok = (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])
    ok &= ((s >= 0) & (s < N) & (t >= 0) & (t < M)).all(1)
    ok &= (s[:, 0] != s[:, 1]) & (s[:, 0] != s[:, 2]) & (s[:, 1] != s[:, 2]) & (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])
    p = src_b[np.clip(s, 0, N - 1), :3].astype(np.float64)
    q = tgt_b[np.clip(t, 0, M - 1), :3].astype(np.float64)
    ok &= np.isfinite(p).all((1, 2)) & np.isfinite(q).all((1, 2))
    with np.errstate(all="ignore"):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            lp, lq = _len(p[:, j] - p[:, i]), _len(q[:, j] - q[:, i])
            ok &= (lp > 0) & (lq > 0) & (np.minimum(lp, lq) >= edge_ratio * np.maximum(lp, lq))
        Th, lwp, lwq = triad(p, q)
        ok &= (lwp > 0) & np.isfinite(lwp) & (lwq > 0) & np.isfinite(lwq) & np.isfinite(Th).all(1)
    T[ok] = Th[ok]
    return T, ok, rows


def pair_points(src_b, tgt_b, ps, pt, n):
    """-> (p [n,3], q [n,3] fp64, use bool [n], err bits): the pairs that can be inliers."""
    N, M = len(src_b), len(tgt_b)
    s, t = ps[:n], pt[:n]
    inr = (s >= 0) & (s < N) & (t >= 0) & (t < M)
    p = src_b[np.clip(s, 0, N - 1), :3].astype(np.float64)
    q = tgt_b[np.clip(t, 0, M - 1), :3].astype(np.float64)
    fin = np.isfinite(p).all(1) & np.isfinite(q).all(1)
    err = (ERR_PAIR if (~inr).any() else 0) | (ERR_NONFINITE if (inr & ~fin).any() else 0)
    return p, q, inr & fin, err


def d2(T, p, q):
    """T [12] or [H,12]; p, q [m,3] -> d2 [m] or [H,m]: e = (R p + t) - q as registration.transform_points states R p + t."""
    T = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        e = [(((T[..., 4 * a, None] * p[:, 0] + T[..., 4 * a + 1, None] * p[:, 1]) + T[..., 4 * a + 2, None] * p[:, 2]) + T[..., 4 * a + 3, None]) - q[:, a]
             for a in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def ransac(src, tgt, pair_src, pair_tgt, threshold, H, seed=0, edge_ratio=0.9, count=None):
    """pn2_corr_ransac on numpy inputs: src [B,N,lds], tgt [B,M,ldt] float32, pairs int64 [B,N].  Returns a dict: T [B,12], hyp
    [B,H,12], hyp_count int32 [B,H] (-1: invalid), best_h int32 [B], best_count int64 [B], status int32 [B], err."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    B, N = src.shape[:2]
    ns = np.full(B, N, np.int64) if count is None else np.clip(np.asarray(count, np.int64), 0, N)
    thr2 = float(threshold) * float(threshold)
    out = dict(T=np.tile(IDENTITY, (B, 1)), hyp=np.full((B, H, 12), np.nan), hyp_count=np.full((B, H), -1, np.int32), best_h=np.full(B, -1, np.int32),
               best_count=np.zeros(B, np.int64), status=np.zeros(B, np.int32), err=0)
    for b in range(B):
        n = int(ns[b])
        T, valid, _ = hypotheses(src[b], tgt[b], pair_src[b], pair_tgt[b], n, seed, b, H, edge_ratio)
        p, q, use, err = pair_points(src[b], tgt[b], pair_src[b], pair_tgt[b], n)
        out["err"] |= err
        counts = np.zeros(H, np.int64)
        for h0 in range(0, H, 64):
            counts[h0:h0 + 64] = (d2(T[h0:h0 + 64], p[use], q[use]) <= thr2).sum(1)
        out["hyp"][b] = T
        out["hyp_count"][b] = np.where(valid, counts, -1)
        if valid.any():
            h = int(np.flatnonzero(valid)[np.argmax(counts[valid])])          # (argmax: the first among equals, i.e. the lowest h)
            out["best_h"][b], out["best_count"][b] = h, counts[h]
        if not valid.any() or out["best_count"][b] < 3:
            out["status"][b] = NONE
            out["err"] |= ERR_NONE
        else:
            out["T"][b] = T[out["best_h"][b]]
    return out


def inliers(src_b, tgt_b, ps, pt, n, T, threshold):
    """-> (bool [n], p [n,3], q [n,3], d2 [n]) of one cloud under T."""
    p, q, use, _ = pair_points(src_b, tgt_b, ps, pt, n)
    dd = d2(T, p, q)
    with np.errstate(invalid="ignore"):
        return use & (dd <= float(threshold) * float(threshold)), p, q, dd


def refit_sums(p, q, dd):
    """The seventeen sums over inlier rows p, q [m,3] with their d2 -> (sums [17], abs_sums [17])."""
    Tm = refit_terms(p, q, dd)
    return Tm.sum(0), np.abs(Tm).sum(0)


def refit_terms(p, q, dd):
    """-> [m,17]: the seventeen terms of every inlier pair, in row order -- what ``refit_sums`` adds up."""
    cols = [np.ones(len(p))] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + [p[:, a] * q[:, c] for a in range(3) for c in range(3)] + [dd]
    return np.stack(cols, 1) if len(p) else np.zeros((0, SUMS))


def horn_matrix(S):
    """sums [17] -> (N [4,4], n): the header's S_ab and N(S)."""
    S = [float(v) for v in S]
    n = S[0]
    with np.errstate(all="ignore"):
        C = [[np.float64(S[7 + 3 * a + e]) - (np.float64(S[1 + a]) * S[4 + e]) / np.float64(n) for e in range(3)] for a in range(3)]
    A = np.zeros((4, 4))
    A[0, 0] = (C[0][0] + C[1][1]) + C[2][2]
    A[1, 1] = (C[0][0] - C[1][1]) - C[2][2]
    A[2, 2] = (C[1][1] - C[0][0]) - C[2][2]
    A[3, 3] = (C[2][2] - C[0][0]) - C[1][1]
    A[0, 1] = A[1, 0] = C[1][2] - C[2][1]
    A[0, 2] = A[2, 0] = C[2][0] - C[0][2]
    A[0, 3] = A[3, 0] = C[0][1] - C[1][0]
    A[1, 2] = A[2, 1] = C[0][1] + C[1][0]
    A[1, 3] = A[3, 1] = C[2][0] + C[0][2]
    A[2, 3] = A[3, 2] = C[1][2] + C[2][1]
    return A, n


def jacobi4(A, sweeps=SWEEPS):
    """csrc/sym_eig4.h on one symmetric 4 x 4 -> (diag [4] unsorted, V [4,4] columns, off: the off-diagonal norm after each sweep)."""
    A = np.array(A, np.float64)
    V = np.eye(4)
    off = []
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq = A[p, q]
                on = apq != 0
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = -t if theta < 0 else t
                t = t if on else 0.0
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * (apq if on else 0.0)
                if on:
                    A[p, p], A[q, q] = A[p, p] - h, A[q, q] + h
                A[p, q] = A[q, p] = 0.0
                for r in range(4):
                    if r in (p, q):
                        continue
                    rp, rq = A[r, p], A[r, q]
                    A[r, p] = A[p, r] = c * rp - s * rq if on else rp
                    A[r, q] = A[q, r] = s * rp + c * rq if on else rq
                for k in range(4):
                    vp, vq = V[k, p], V[k, q]
                    V[k, p] = c * vp - s * vq if on else vp
                    V[k, q] = s * vp + c * vq if on else vq
            off.append(float(np.sqrt(sum(A[p, q] ** 2 for p, q in PAIRS))))
    return np.diag(A).copy(), V, off


def largest(diag, V):
    """The column of the largest diagonal entry, the first among equals (strict >)."""
    best, u = diag[0], V[:, 0].copy()
    for c in range(1, 4):
        if diag[c] > best:
            best, u = diag[c], V[:, c].copy()
    return u


def quat_to_T(u, S):
    """The header's normalisation, sign, R and t from the eigenvector u and the sums S -> T [12]."""
    n = float(S[0])
    with np.errstate(all="ignore"):
        ln = np.sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3])
        w, x, y, z = (u[k] / ln for k in range(4))
        if w < 0:
            w, x, y, z = -w, -x, -y, -z
        R = np.zeros((3, 4))
        R[0, 0] = ((w * w + x * x) - y * y) - z * z
        R[0, 1] = 2.0 * (x * y - w * z)
        R[0, 2] = 2.0 * (x * z + w * y)
        R[1, 0] = 2.0 * (x * y + w * z)
        R[1, 1] = ((w * w - x * x) + y * y) - z * z
        R[1, 2] = 2.0 * (y * z - w * x)
        R[2, 0] = 2.0 * (x * z - w * y)
        R[2, 1] = 2.0 * (y * z + w * x)
        R[2, 2] = ((w * w - x * x) - y * y) + z * z
        m = [np.float64(S[1 + a]) / n for a in range(3)]
        for a in range(3):
            R[a, 3] = np.float64(S[4 + a]) / n - ((R[a, 0] * m[0] + R[a, 1] * m[1]) + R[a, 2] * m[2])
    return R.reshape(12)


def horn(S):
    """The part of a refit round after the sums -> (T [12] or None, degenerate)."""
    A, n = horn_matrix(S)
    diag, V, _ = jacobi4(A)
    T = quat_to_T(largest(diag, V), S)
    if n < 3 or not np.isfinite(T).all():
        return None, True
    return T, False


def rmse_of(S):
    return float(np.sqrt(S[16] / S[0])) if S[0] > 0 else 0.0


def refit(src_b, tgt_b, ps, pt, n, T, threshold):
    """One pn2_corr_refit round of one cloud -> dict(T, sums, abs_sums, count, rmse, degenerate, inlier)."""
    inl, p, q, dd = inliers(src_b, tgt_b, ps, pt, n, T, threshold)
    S, A = refit_sums(p[inl], q[inl], dd[inl])
    Tn, deg = horn(S)
    return dict(T=np.asarray(T, np.float64).copy() if deg else Tn, sums=S, abs_sums=A, count=int(inl.sum()), rmse=rmse_of(S), degenerate=deg, inlier=inl)


def kabsch(p, q):
    """SVD-Kabsch, the textbook route (reflection corrected): the rigid T [12] that takes rows p onto rows q in the least-squares sense."""
    pm, qm = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - pm).T @ (q - qm))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return np.concatenate([R, (qm - R @ pm)[:, None]], 1).reshape(12)


def apply(T, p):
    T = np.asarray(T, np.float64).reshape(3, 4)
    return p @ T[:, :3].T + T[:, 3]


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(degrees)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


_scene = {}


def bump_scene(M=3072, seed=11):
    """The end-to-end scene (made once, read-only): M points on the height field of 12 Gaussian bumps over [-2,2]^2 (random
    centres, amplitudes in [-0.5, 0.5], widths in [0.2, 0.5]) with analytic unit normals (pointing up).  target = the rows with
    x > -0.8; source = the rows with x < 0.8, permuted, rotated 140 degrees about (1,2,3) and translated by (0.7, -1.1, 0.4).
    Returns a dict: source / source_normals / target / target_normals float32 [.,3], T_true [12] fp64 (source -> target frame),
    truth fp64 [N,3] (every source row's true position in the target frame)."""
    key = (M, seed)
    if key not in _scene:
        rng = np.random.default_rng(seed)
        cen, amp, wid = rng.uniform(-2, 2, (12, 2)), rng.uniform(-0.5, 0.5, 12), rng.uniform(0.2, 0.5, 12)
        xy = rng.uniform(-2, 2, (M, 2))
        d = xy[:, None, :] - cen[None]
        g = amp * np.exp(-(d ** 2).sum(2) / (2 * wid ** 2))
        z = g.sum(1)
        grad = (-(d / wid[None, :, None] ** 2) * g[:, :, None]).sum(1)
        pts = np.concatenate([xy, z[:, None]], 1)
        nrm = np.concatenate([-grad, np.ones((M, 1))], 1)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        tsel = pts[:, 0] > -0.8
        ssel = np.flatnonzero(pts[:, 0] < 0.8)
        ssel = ssel[rng.permutation(len(ssel))]
        R, t = rotation((1, 2, 3), 140.0), np.array([0.7, -1.1, 0.4])
        source = (pts[ssel] @ R.T + t).astype(np.float32)            # the source frame: a moved copy
        Rt = R.T
        T_true = np.concatenate([Rt, (-Rt @ t)[:, None]], 1).reshape(12)
        out = dict(source=source, source_normals=(nrm[ssel] @ R.T).astype(np.float32), target=pts[tsel].astype(np.float32),
                   target_normals=nrm[tsel].astype(np.float32), T_true=T_true, truth=apply(T_true, source.astype(np.float64)))
        for v in out.values():
            v.setflags(write=False)
        _scene[key] = out
    return _scene[key]


EPS = 2.0 ** -52
C_HORN = 40.0                    # tests/test_corr_ransac_cpu.py measures the reference's own error in these units and states the margin


def horn_bound(S):
    """The perturbation scale of the solve of sums S: eps * ||N||_F / gap, gap = the distance between N's two largest eigenvalues
    (numpy.linalg.eigh) -> (scale, gap / ||N||_F, eigh's top eigenvector)."""
    A, _ = horn_matrix(S)
    lam, vec = np.linalg.eigh(A)
    nrm = float(np.linalg.norm(A))
    gap = float(lam[3] - lam[2])
    return EPS * nrm / gap, gap / nrm, vec[:, 3]


def transform_tolerance(S, abs_sums=None):
    """What two correct solves of the same sums may differ by, entry by entry of T [12]: the eigenvector moves by at most
    C_HORN * scale; an entry of R is quadratic in the unit quaternion (|dR| <= 4 |du|), and t = q_mean - R p_mean moves by
    |dR| * |p_mean|_1 on top of one rounding of its own magnitude.  With ``abs_sums`` (a solve by another route, from the points
    and not from these sums): N itself then carries the rounding of S_ab = sum p_a q_b - (sum p_a)(sum q_b) / n, which cancels
    when the centroids are far from the origin: ||N||_F grows by the magnitudes that cancel, max sum |p_a q_b| + max |sum p| max
    |sum q| / n."""
    scale, _, _ = horn_bound(S)
    if abs_sums is not None:
        A, _ = horn_matrix(S)
        scale *= 1.0 + (np.max(abs_sums[7:16]) + np.abs(S[1:4]).max() * np.abs(S[4:7]).max() / S[0]) / float(np.linalg.norm(A))
    du = C_HORN * scale
    pm = np.abs(np.asarray(S[1:4]) / S[0]).sum()
    qm = np.abs(np.asarray(S[4:7]) / S[0]).max()
    tol = np.full((3, 4), 4.0 * du + 4 * EPS)
    tol[:, 3] = 4.0 * du * pm + 8 * EPS * (pm + qm)
    return tol.reshape(12)
