"""The plane rule of include/pn2.h ("plane RANSAC") in numpy: what pn2_plane_ransac, pn2_plane_refit and pn2_plane_classify must write.

Every floating-point term is the fp64 statement of the header, one rounding per operation (numpy never fuses).  The sampler is
integer arithmetic mod 2^64 on Python integers (``sample``) and on uint64 arrays (``sample_rows``); the two are compared in
tests/test_plane_cpu.py.  ``refit_sums`` adds the ten terms with numpy's sum -- the device adds the SAME terms in another order, so
``abs_sums`` (the sums of their magnitudes) is what a test scales its bound by -- and ``refit_finish`` is the part after the sums,
usable on the DEVICE's own sums.  The eigen-solver is tests/normals_ref.py's restatement of csrc/sym_eig3.h."""
import math

import numpy as np

import normals_ref

NONE, DEGENERATE, SMALL = 1, 2, 4
ERR_NONFINITE, ERR_NONE = 1, 2
MASK = (1 << 64) - 1
GOLDEN, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
SWEEPS = 6                       # PN2_PCA_SWEEPS


def sample(seed, b, h, j, n):
    """Row j of hypothesis h of cloud b among n rows, on Python integers."""
    x = (seed * GOLDEN + (b << 40 | h << 8 | j)) & MASK
    x ^= x >> 30
    x = x * MUL1 & MASK
    x ^= x >> 27
    x = x * MUL2 & MASK
    x ^= x >> 31
    return ((x >> 32) * n) >> 32


def sample_rows(seed, b, H, n):
    """[H,3] int64: the three rows of every hypothesis of cloud b (uint64 arithmetic wraps as the rule says)."""
    with np.errstate(over="ignore"):
        word = np.uint64(b << 40) | (np.arange(H, dtype=np.uint64)[:, None] << np.uint64(8)) | np.arange(3, dtype=np.uint64)[None, :]
        x = np.uint64(seed * GOLDEN & MASK) + word
        x ^= x >> np.uint64(30)
        x *= np.uint64(MUL1)
        x ^= x >> np.uint64(27)
        x *= np.uint64(MUL2)
        x ^= x >> np.uint64(31)
        return (((x >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def unit_axis(axis):
    a = np.asarray(axis, np.float64)
    return a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def flip(n, axis):
    """n [.,3] negated where n . axis < 0, or == 0 with a negative first non-zero component."""
    t = (n[..., 0] * axis[0] + n[..., 1] * axis[1]) + n[..., 2] * axis[2]
    lead = np.where(n[..., 0] != 0, n[..., 0], np.where(n[..., 1] != 0, n[..., 1], n[..., 2]))
    neg = (t < 0) | ((t == 0) & (lead < 0))
    return np.where(neg[..., None], -n, n)


def takes_part(N, n, assign_b):
    part = np.arange(N) < n
    return part if assign_b is None else part & (assign_b < 0)


def residual(plane, p):
    """plane [4] or [H,4], p [m,3] fp64 -> r [m] or [H,m]: ((n_x x + n_y y) + n_z z) + d."""
    P = np.asarray(plane, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((P[..., 0, None] * p[:, 0] + P[..., 1, None] * p[:, 1]) + P[..., 2, None] * p[:, 2]) + P[..., 3, None]


def hypotheses(pts_b, n, part, seed, b, H, axis, cos_max):
    """-> (planes [H,4] fp64, NaN rows for invalid hypotheses; valid [H] bool; rows [H,3])."""
    p = pts_b[:, :3].astype(np.float64)
    rows = sample_rows(seed, b, H, n)
    planes = np.full((H, 4), np.nan)
    if n == 0:
        return planes, np.zeros(H, bool), rows
    r0, r1, r2 = rows.T
    ok = (r0 != r1) & (r0 != r2) & (r1 != r2) & part[r0] & part[r1] & part[r2]
    ok &= np.isfinite(p[r0]).all(1) & np.isfinite(p[r1]).all(1) & np.isfinite(p[r2]).all(1)
    with np.errstate(all="ignore"):
        a, c = p[r1] - p[r0], p[r2] - p[r0]
        cr = np.stack([a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]], 1)
        l2 = (cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2]
        ok &= (l2 > 0) & np.isfinite(l2)
        nrm = flip(cr / np.sqrt(l2)[:, None], axis)
        t = (nrm[:, 0] * axis[0] + nrm[:, 1] * axis[1]) + nrm[:, 2] * axis[2]
        ok &= ~(t < cos_max)
        d = -((nrm[:, 0] * p[r0, 0] + nrm[:, 1] * p[r0, 1]) + nrm[:, 2] * p[r0, 2])
    planes[ok, :3], planes[ok, 3] = nrm[ok], d[ok]
    return planes, ok, rows


def ransac(pts, threshold, H, seed=0, axis=(0, 0, 1), cos_max=0.0, n_points=None, assign=None):
    """pn2_plane_ransac on numpy inputs: pts [B,N,ld] float32, assign int32 [B,N] or None (read only).  Returns a dict: plane [B,4],
    hyp_count int32 [B,H] (-1: invalid), hyp [B,H,4], best_h int32 [B], best_count int64 [B], status int32 [B], err."""
    pts = np.asarray(pts, np.float32)
    B, N = pts.shape[:2]
    ns = np.full(B, N, np.int64) if n_points is None else np.clip(np.asarray(n_points, np.int64), 0, N)
    ax = unit_axis(axis)
    out = dict(plane=np.zeros((B, 4)), hyp_count=np.full((B, H), -1, np.int32), hyp=np.full((B, H, 4), np.nan), best_h=np.full(B, -1, np.int32),
               best_count=np.zeros(B, np.int64), status=np.zeros(B, np.int32), err=0)
    for b in range(B):
        n = int(ns[b])
        part = takes_part(N, n, None if assign is None else assign[b])
        p = pts[b, :, :3].astype(np.float64)
        finite = np.isfinite(p).all(1)
        if (part & ~finite).any():
            out["err"] |= ERR_NONFINITE
        planes, valid, _ = hypotheses(pts[b], n, part, seed, b, H, ax, cos_max)
        use = part & finite
        counts = np.zeros(H, np.int64)
        for h0 in range(0, H, 64):                                 # (blocks of hypotheses: [64, n] residuals at a time)
            with np.errstate(invalid="ignore"):
                counts[h0:h0 + 64] = (np.abs(residual(planes[h0:h0 + 64], p[use])) <= threshold).sum(1)
        out["hyp"][b] = planes
        out["hyp_count"][b] = np.where(valid, counts, -1)
        if valid.any():
            h = int(np.flatnonzero(valid)[np.argmax(counts[valid])])          # (argmax: the first among equals, i.e. the lowest h)
            out["best_h"][b], out["best_count"][b] = h, counts[h]
        if not valid.any() or out["best_count"][b] < 3:
            out["status"][b] = NONE
            out["err"] |= ERR_NONE
        else:
            out["plane"][b] = planes[out["best_h"][b]]
    return out


def inliers(pts_b, n, assign_b, plane, threshold):
    """bool [N]: the rows of one cloud that take part, are finite and have |r| <= threshold."""
    p = pts_b[:, :3].astype(np.float64)
    use = takes_part(len(p), n, assign_b) & np.isfinite(p).all(1)
    with np.errstate(invalid="ignore"):
        return use & (np.abs(residual(plane, p)) <= threshold)


def refit_sums(pts_b, inl, plane):
    """-> (sums [10], abs_sums [10]): count, sum q, sum q q^T (xx, xy, xz, yy, yz, zz) over the inliers, q = double(p) - (-d) n."""
    T = refit_terms(pts_b, inl, plane)
    return T.sum(0), np.abs(T).sum(0)


def refit_terms(pts_b, inl, plane):
    """-> [m,10]: the ten terms of every inlier, in row order -- what ``refit_sums`` adds up."""
    P = np.asarray(plane, np.float64)
    s = -P[3] * P[:3]
    q = pts_b[inl, :3].astype(np.float64) - s
    cols = [np.ones(len(q)), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2], q[:, 1] * q[:, 1],
            q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]]
    return np.stack(cols, 1) if len(q) else np.zeros((0, 10))


def sym_eig3(C6):
    """csrc/sym_eig3.h on one matrix (xx, xy, xz, yy, yz, zz) -> (l0, l1, l2, u [3]): the smallest diagonal entry, the first among equals."""
    diag, V, _ = normals_ref.jacobi_eig3(np.asarray(C6, np.float64)[None], SWEEPS)
    xx, yy, zz = (float(v) for v in diag[0])
    y_lt_x = yy < xx
    m01 = yy if y_lt_x else xx
    z_lt = zz < m01
    col = 2 if z_lt else (1 if y_lt_x else 0)
    hi01 = xx if y_lt_x else yy
    l2 = zz if zz > hi01 else hi01
    l1 = m01 if z_lt else (hi01 if zz > hi01 else zz)
    return (zz if z_lt else m01), l1, l2, V[0][:, col].copy()


def refit_finish(sums, plane, axis=(0, 0, 1)):
    """The part of a refit round after the sums -> (plane' [4], rmse or None, degenerate)."""
    S = [float(v) for v in sums]
    P = [float(v) for v in plane]
    ax = unit_axis(axis)
    count = S[0]
    if count < 3:
        return np.array(P), None, True
    s = [-P[3] * P[0], -P[3] * P[1], -P[3] * P[2]]
    m = [S[1] / count, S[2] / count, S[3] / count]
    C6 = [S[4] / count - m[0] * m[0], S[5] / count - m[0] * m[1], S[6] / count - m[0] * m[2], S[7] / count - m[1] * m[1],
          S[8] / count - m[1] * m[2], S[9] / count - m[2] * m[2]]
    l0, l1, l2, u = sym_eig3(C6)
    if not l1 > 0 or not (np.isfinite(u).all() and math.isfinite(l0)):
        return np.array(P), None, True
    u = flip(u, ax)
    d = -((u[0] * (s[0] + m[0]) + u[1] * (s[1] + m[1])) + u[2] * (s[2] + m[2]))
    return np.array([u[0], u[1], u[2], d]), math.sqrt(max(l0, 0.0)), False


def classify(pts_b, n, assign_b, plane, threshold):
    """-> (dist float32 [N] with NaN beyond n and on rows that are not finite, inlier bool [N])."""
    p = pts_b[:, :3].astype(np.float64)
    finite = np.isfinite(p).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(finite, residual(plane, p), np.nan)
        dist = r.astype(np.float32)
    dist[n:] = np.nan
    return dist, inliers(pts_b, n, assign_b, plane, threshold)


def fit_plane(pts, threshold, H=256, seed=0, axis=(0, 0, 1), cos_max=0.0, refine=2, n_points=None, assign=None, plane_id=0, min_inliers=0):
    """The whole rule on numpy inputs: ransac, ``refine`` refit rounds, classify.  ``assign`` (int32 [B,N] or None) is WRITTEN as the
    device writes it.  Returns ransac's dict with plane the final plane and plane0 the selected hypothesis, rmse [B] (0 where never
    written), sums / abs_sums [B,10] of the last round, count int64 [B] (-1 where not written), dist float32 [B,N] (NaN where not
    written), inlier bool [B,N] (the final inliers)."""
    pts = np.asarray(pts, np.float32)
    B, N = pts.shape[:2]
    ns = np.full(B, N, np.int64) if n_points is None else np.clip(np.asarray(n_points, np.int64), 0, N)
    out = ransac(pts, threshold, H, seed, axis, cos_max, n_points, assign)
    out.update(plane0=out["plane"].copy(), rmse=np.zeros(B), sums=np.zeros((B, 10)), abs_sums=np.zeros((B, 10)), count=np.full(B, -1, np.int64),
               dist=np.full((B, N), np.nan, np.float32), inlier=np.zeros((B, N), bool))
    for b in range(B):
        if out["status"][b] & NONE:
            continue
        a_b, n = None if assign is None else assign[b], int(ns[b])
        for _ in range(refine):
            inl = inliers(pts[b], n, a_b, out["plane"][b], threshold)
            out["sums"][b], out["abs_sums"][b] = refit_sums(pts[b], inl, out["plane"][b])
            plane, rmse, degenerate = refit_finish(out["sums"][b], out["plane"][b], axis)
            if degenerate:
                out["status"][b] |= DEGENERATE
            else:
                out["plane"][b], out["rmse"][b] = plane, rmse
        out["dist"][b], out["inlier"][b] = classify(pts[b], n, a_b, out["plane"][b], threshold)
        out["count"][b] = out["inlier"][b].sum()
        if out["count"][b] < min_inliers:
            out["status"][b] |= SMALL
        elif assign is not None:
            assign[b][out["inlier"][b]] = plane_id
    return out


def tilt_degrees(plane, axis=(0, 0, 1)):
    n = np.asarray(plane, np.float64)[..., :3]
    return np.degrees(np.arccos(np.clip(n @ unit_axis(axis), -1.0, 1.0)))
