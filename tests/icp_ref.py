"""The ICP rule of include/pn2.h ("ICP step") in numpy: what pn2_icp_step must write.

The search is tests/grid_knn_ref.py's at K = 1; every term is the fp64 statement of the header, one rounding per operation (numpy
never fuses); ``sums`` is numpy's sum of those terms -- the device adds the SAME terms in another order, so ``abs_sums`` (the sum of
their magnitudes) is what a test scales its bound by.  ``solve`` and ``update`` are the header's Cholesky and rotation update on
Python floats (IEEE fp64), usable on their own: a test applies ``update`` to the DEVICE's ``x``."""
import math

import numpy as np

import grid_knn_ref as R

POINT, PLANE = 0, 1
EVAL_ONLY = 1
CONVERGED, SINGULAR = 1, 2
ERR_QUERY, ERR_SINGULAR, ERR_NONFINITE = 1, 2, 4
AXES = np.eye(3)


def transform(T, src):
    """T [12] or [3,4] fp64, src [n, >=3] float32 -> p [n,3] fp64: p_a = ((R_a0 s_0 + R_a1 s_1) + R_a2 s_2) + t_a."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    s = np.asarray(src, np.float32)[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[a, 0] * s[:, 0] + T[a, 1] * s[:, 1]) + T[a, 2] * s[:, 2]) + T[a, 3] for a in range(3)], -1)


def terms(p, e, n):
    """p, e, n [m,3] fp64 -> [m,28]: J_k J_l for k <= l row-major, J_k r, r r with r = (n_x e_x + n_y e_y) + n_z e_z, J = (p x n, n)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
        J = [p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2]]
        cols = [J[k] * J[l] for k in range(6) for l in range(k, 6)] + [J[k] * r for k in range(6)] + [r * r]
    return np.stack(cols, -1) if len(r) else np.zeros((0, 28))


def matrices(sums):
    """sums [28] -> A [6,6] symmetric, b [6], E."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    return A + np.triu(A, 1).T, np.array(sums[21:27], np.float64), float(sums[27])


def solve(sums, count, metric):
    """-> (x [6], singular, nonfinite): A x = -b by Cholesky in index order; singular iff count < 6 (PLANE) / 3 (POINT) or a pivot
    is <= 2^-40 times its diagonal entry or is not finite.  x = 0 when singular."""
    A, b, _ = matrices(np.asarray(sums, np.float64))
    if not np.isfinite(np.asarray(sums)).all():
        return np.zeros(6), True, True
    bad = count < (6 if metric == PLANE else 3)
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        ajj = float(A[j, j])
        d = ajj
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if d <= 2.0 ** -40 * ajj or not math.isfinite(d):
            bad = True
            break
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            s = float(A[j, i])
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    if bad:
        return np.zeros(6), True, False
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = -float(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return np.array(x), False, False


def update(T, x):
    """T [12] fp64, x [6] -> (T' [12], theta, |v|): D = (I + a [w]x) + b [w]x^2, R <- D R, t <- D t + v."""
    T = [float(v) for v in np.asarray(T, np.float64).reshape(12)]
    w0, w1, w2, v = float(x[0]), float(x[1]), float(x[2]), [float(x[3]), float(x[4]), float(x[5])]
    th = math.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    tt = th * th
    if th < 2.0 ** -20:
        a, bb = 1.0 - tt / 6.0, 0.5 - tt / 24.0
    else:
        a, bb = math.sin(th) / th, (1.0 - math.cos(th)) / tt
    K = [0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0]
    K2 = [-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2, w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2, w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)]
    D = [((1.0 if q % 4 == 0 else 0.0) + a * K[q]) + bb * K2[q] for q in range(9)]
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[i * 4 + j] = (D[i * 3] * T[j] + D[i * 3 + 1] * T[4 + j]) + D[i * 3 + 2] * T[8 + j]
        out[i * 4 + 3] = ((D[i * 3] * T[3] + D[i * 3 + 1] * T[7]) + D[i * 3 + 2] * T[11]) + v[i]
    return np.array(out), th, math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def step_terms(p, tgt_b, normals_b, j, metric):
    """p [n,3] fp64 (the transformed source), j int64 [n] (the K = 1 answers, M: nobody) -> (t [m,28], rows int64 [m], part bool [n]):
    the terms a step adds up, the source row each of them comes from (POINT: three terms per row, axis by axis) and the rows that
    take part (PLANE: matched to a target whose normal is finite and not zero)."""
    M = len(tgt_b)
    part = j < M
    jj = np.where(part, j, 0)
    e = p - tgt_b[jj, :3].astype(np.float64)
    if metric == PLANE:
        nv = normals_b[jj, :3].astype(np.float64)
        part = part & np.isfinite(nv).all(-1) & ~(nv == 0).all(-1)
        return terms(p[part], e[part], nv[part]), np.flatnonzero(part), part
    t = np.concatenate([terms(p[part], e[part], np.broadcast_to(AXES[a], (int(part.sum()), 3))) for a in range(3)])
    return t, np.tile(np.flatnonzero(part), 3), part


def icp_step(src, tgt, normals, T, status, iters, max_d2, origin, cell, metric, flags=0, tol_rot=0.0, tol_trans=0.0, n_src=None, n_tgt=None):
    """One pn2_icp_step on numpy inputs: src [B,N,ld], tgt [B,M,ld] float32, normals [B,M,>=3] float32 (None for POINT), T [B,12]
    fp64, status / iters int32 [B] -- none of them written to.  Returns a dict: T, x [B,6], status, iters, sums [B,28], abs_sums
    [B,28] (the sums of the terms' magnitudes), count int64 [B], corr int64 [B,N] (-1 where the call does not write), touched bool
    [B] (clouds that are not frozen), err."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    B, N = src.shape[:2]
    M = tgt.shape[1]
    ev = bool(flags & EVAL_ONLY)
    ns = np.full(B, N, np.int64) if n_src is None else np.clip(np.asarray(n_src, np.int64), 0, N)
    out = dict(T=np.array(T, np.float64).reshape(B, 12), x=np.full((B, 6), np.nan), status=np.array(status, np.int32), iters=np.array(iters, np.int32),
               sums=np.full((B, 28), np.nan), abs_sums=np.zeros((B, 28)), count=np.full(B, -1, np.int64),
               corr=np.full((B, N), -1, np.int64), touched=np.zeros(B, bool), err=0)
    for b in range(B):
        if not ev and out["status"][b] & (CONVERGED | SINGULAR):
            continue
        out["touched"][b] = True
        n = int(ns[b])
        p = transform(out["T"][b], src[b, :n])
        j = np.full(n, M, np.int64)
        if n:
            with np.errstate(invalid="ignore", over="ignore"):
                g = R.grid_knn(p.astype(np.float32)[None], tgt[b:b + 1], 1, max_d2, origin, cell, n_cand=None if n_tgt is None else n_tgt[b:b + 1])
            j = g["idx"][0, :, 0]
            if g["err_query"]:
                out["err"] |= ERR_QUERY
        out["corr"][b, :n] = j
        t, _, part = step_terms(p, tgt[b], None if metric == POINT else np.asarray(normals, np.float32)[b], j, metric)
        out["sums"][b], out["abs_sums"][b], out["count"][b] = t.sum(0), np.abs(t).sum(0), part.sum()
        if ev:
            continue
        x, singular, nonfinite = solve(out["sums"][b], out["count"][b], metric)
        if not np.isfinite(out["T"][b]).all():
            x, singular, nonfinite = np.zeros(6), True, True
        out["x"][b] = x
        if singular:
            out["status"][b] |= SINGULAR
            out["err"] |= ERR_NONFINITE if nonfinite else ERR_SINGULAR
            continue
        out["T"][b], th, step = update(out["T"][b], x)
        out["iters"][b] += 1
        if th <= tol_rot and step <= tol_trans:
            out["status"][b] |= CONVERGED
    return out


def icp(src, tgt, normals, T, max_d2, origin, cell, metric, iterations, tol_rot, tol_trans, n_src=None, n_tgt=None):
    """``iterations`` steps from T [B,12] with status and iters zero -> the last step's dict (its T, status, iters are the loop's)
    with ``last_sums``: per cloud the sums of the last step that cloud took part in."""
    B = np.asarray(src).shape[0]
    T, status, iters = np.array(T, np.float64).reshape(B, 12), np.zeros(B, np.int32), np.zeros(B, np.int32)
    last = np.full((B, 28), np.nan)
    for _ in range(iterations):
        o = icp_step(src, tgt, normals, T, status, iters, max_d2, origin, cell, metric, 0, tol_rot, tol_trans, n_src, n_tgt)
        last[o["touched"]] = o["sums"][o["touched"]]
        T, status, iters = o["T"], o["status"], o["iters"]
        if (status != 0).all():
            break
    o["last_sums"] = last
    return o


def rotation(axis, angle):
    """Rodrigues in fp64: the rotation by ``angle`` about ``axis``."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


PLANTED_R = rotation((1, 2, 3), math.radians(3.0))
PLANTED_T = np.array([0.05, -0.02, 0.03])
PLANTED = np.concatenate([PLANTED_R, PLANTED_T[:, None]], 1).reshape(12)
SHEETS_MAX_DIST = 0.5
_sheets = {}


def sheets_pair():
    """(src [1,1024,3], tgt [1,2048,3], normals [1,2048,3]) float32, read-only: the target is three mutually tilted wavy sheets
    (z = 0.15 sin(1.3 u + k) cos(1.1 v) over [-2,2]^2 in three frames that are 60 degrees and more apart) with their analytic unit
    normals; the source is every second target point under the INVERSE of the planted transform, rounded to float32 -- no other
    noise, so registering source to target recovers PLANTED."""
    if not _sheets:
        rng = np.random.default_rng(77)
        pts, nrm = [], []
        for k, (axis, angle) in enumerate((((1, 0, 0), 0.0), ((1, 0.3, 0), 1.2), ((0.2, 1, 0), -1.3))):
            F = rotation(axis, angle)                              # columns: the sheet's u, v and height axes
            m = 683 if k < 2 else 682
            u, v = rng.uniform(-2, 2, m), rng.uniform(-2, 2, m)
            h = 0.15 * np.sin(1.3 * u + k) * np.cos(1.1 * v)
            hu, hv = 0.15 * 1.3 * np.cos(1.3 * u + k) * np.cos(1.1 * v), -0.15 * 1.1 * np.sin(1.3 * u + k) * np.sin(1.1 * v)
            local = np.stack([u, v, h + 0.4 * k], -1)
            n = np.stack([-hu, -hv, np.ones(m)], -1)
            pts.append(local @ F.T)
            nrm.append((n / np.linalg.norm(n, axis=1, keepdims=True)) @ F.T)
        tgt = np.concatenate(pts).astype(np.float32)
        order = rng.permutation(len(tgt))
        tgt, normals = tgt[order], np.concatenate(nrm).astype(np.float32)[order]
        src = ((tgt[::2].astype(np.float64) - PLANTED_T) @ PLANTED_R).astype(np.float32)       # R^T (q - t), row by row
        for a in (src, tgt, normals):
            a.setflags(write=False)
        _sheets["pair"] = (src[None], tgt[None], normals[None])
    return _sheets["pair"]


_planted = {}


def sheets_reference(metric):
    """The reference's 30-iteration run on the sheets pair from the identity with the default tolerances -> (the loop's dict, e_ref
    = the largest entry of |T - PLANTED|, cond(A) of the last step); computed once per metric."""
    if metric not in _planted:
        src, tgt, normals = sheets_pair()
        m = np.float32(SHEETS_MAX_DIST ** 2)
        o = icp(src, tgt, normals, np.eye(3, 4).reshape(1, 12), m, 0.0, R.default_cell(m), metric, 30, 1e-6, 1e-6 * SHEETS_MAX_DIST)
        A = matrices(o["last_sums"][0])[0]
        _planted[metric] = (o, float(np.abs(o["T"][0] - PLANTED).max()), float(np.linalg.cond(A)))
    return _planted[metric]
