"""The grid kNN rule of include/pn2.h ("grid kNN") in numpy: what pn2_grid_build + pn2_grid_knn must write, bit for bit.

Cells in fp64 (two separately rounded operations), the float32 difference-form distance with each fmaf as "exact sum, one
rounding", a stable lexicographic sort on (d2, index), the (M, +inf) padding, ``count`` and the two error bits; and a brute-force
"K nearest with d2 <= max_d2" in the same arithmetic, which the grid statement EQUALS when the cell is at least
``default_cell(max_d2)`` ("Grid kNN")."""
import numpy as np

ERR_CAND, ERR_QUERY = 1, 2
LIMIT = 1048576.0                      # cells per axis: [-2^20, 2^20)


def default_cell(max_d2):
    """The smallest cell edge that keeps the equality with brute force: sqrt((double)max_d2) * (1 + 2^-20)."""
    return float(np.sqrt(np.float64(np.float32(max_d2))) * (1.0 + 2.0 ** -20))


def disc_cloud(rng, B, M, ld=4):
    """[B, M, ld] float32: a uniform disc of radius 12 (r = 12 sqrt(u), a random angle), z in [-1.5, 1.5); the columns from 3 on are
    not coordinates."""
    r, a = 12.0 * np.sqrt(rng.random((B, M))), 2 * np.pi * rng.random((B, M))
    pts = rng.random((B, M, ld)).astype(np.float32)
    pts[..., 0], pts[..., 1], pts[..., 2] = r * np.cos(a), r * np.sin(a), 3 * rng.random((B, M)) - 1.5
    return pts


def cells(p, origin, cell):
    """p [..., 3] float32 -> (q int64 [..., 3], valid bool [...]): q = floor(((double)p - origin) / cell), valid iff -2^20 <= q < 2^20
    on all three axes (NaN and inf fail).  q is 0 where the row is invalid."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((np.asarray(p, np.float32)[..., :3].astype(np.float64) - np.asarray(origin, np.float64)) / np.asarray(cell, np.float64))
        ok = (q >= -LIMIT) & (q < LIMIT)
    valid = ok.all(-1)
    return np.where(valid[..., None], q, 0.0).astype(np.int64), valid


def fma32(t, d2):
    """fmaf(t, t, d2) for float32 arrays: the exact t * t + d2 rounded ONCE to float32.  t * t is exact in fp64 (48 bits); the fp64
    sum s rounds once, and rounding that again to float32 would round twice -- so the sum is first made "round to odd": where it
    was inexact (two-sum's error term e != 0) and s is even, s moves one ulp towards e.  An odd 53-bit value never sits on a
    float32 tie or on a float32 number, and lies on the same side of each as the exact sum: the second rounding is then the only
    one that matters (53 >= 2 * 24 + 2)."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.asarray(t, np.float32).astype(np.float64) ** 2
        b = np.asarray(d2, np.float32).astype(np.float64)
        s = a + b
        bb = s - a
        e = (a - (s - bb)) + (b - bb)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def dist2(q, p):
    """q [N,3], p [M,3] float32 -> d2 float32 [N,M]: t_a = q_a - p_a; d2 = t_x * t_x; d2 = fmaf(t_y, t_y, d2); d2 = fmaf(t_z, t_z, d2)."""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = [q[:, None, a] - p[None, :, a] for a in range(3)]
        d2 = t[0] * t[0]
    return fma32(t[2], fma32(t[1], d2))


def _select(d2, part, K, M):
    """d2 [N,M] float32, part [N,M] bool -> idx int64 [N,K], dist float32 [N,K], count int32 [N]: the participants in ascending
    (d2, index) order, the first K of them, (M, +inf) in the slots beyond."""
    N = d2.shape[0]
    index = np.broadcast_to(np.arange(M), d2.shape)
    order = np.lexsort((index, np.where(part, d2, np.float32(np.inf)), ~part), axis=-1)[:, :K]      # (last key first)
    took = np.take_along_axis(part, order, -1)
    idx = np.full((N, K), M, np.int64)
    dist = np.full((N, K), np.inf, np.float32)
    w = min(K, M)
    idx[:, :w] = np.where(took, order, M)
    dist[:, :w] = np.where(took, np.take_along_axis(d2, order, -1), np.float32(np.inf))
    return idx, dist, part.sum(-1).astype(np.int32)


def _counts(n, B, full):
    return np.full(B, full, np.int64) if n is None else np.clip(np.asarray(n, np.int64).reshape(B), 0, full)


def grid_knn(query, cand, K, max_d2, origin, cell, n_query=None, n_cand=None):
    """cand [B,M,ld], query [B,N,ld] float32 (None: a self-search) -> dict with idx int64 [B,N,K], dist float32 [B,N,K], count int32
    [B,N], written bool [B,N] (the rows the call writes; the others are -1 / NaN / -1 here and untouched on the device),
    err_build and err_query (the bits pn2_grid_build / pn2_grid_knn OR into their err)."""
    cand = np.asarray(cand, np.float32)
    B, M = cand.shape[:2]
    self_search = query is None
    query = cand if self_search else np.asarray(query, np.float32)
    N = query.shape[1]
    max_d2 = np.float32(max_d2)
    nc = _counts(n_cand, B, M)
    nq = nc if self_search else _counts(n_query, B, N)
    out = dict(idx=np.full((B, N, K), -1, np.int64), dist=np.full((B, N, K), np.nan, np.float32), count=np.full((B, N), -1, np.int32),
               written=np.zeros((B, N), bool), err_build=0, err_query=0)
    for b in range(B):
        cc, cvalid = cells(cand[b], origin, cell)
        cvalid = cvalid & (np.arange(M) < nc[b])
        if not cvalid[:nc[b]].all():
            out["err_build"] |= ERR_CAND
        n = int(nq[b])
        qc, qvalid = cells(query[b, :n], origin, cell)
        if not qvalid.all():
            out["err_query"] |= ERR_QUERY
        near = (np.abs(qc[:, None, :] - cc[None, :, :]) <= 1).all(-1)                      # (a cell outside the grid holds no valid row)
        d2 = dist2(query[b, :n, :3], cand[b, :, :3])
        with np.errstate(invalid="ignore"):
            part = near & cvalid[None, :] & qvalid[:, None] & (d2 <= max_d2)
        out["idx"][b, :n], out["dist"][b, :n], out["count"][b, :n] = _select(d2, part, K, M)
        out["written"][b, :n] = True
    return out


def brute_knn(query, cand, K, max_d2, n_query=None, n_cand=None):
    """The brute-force statement in the same arithmetic: of the first n_cand candidates those with d2 <= max_d2, the first K in
    ascending (d2, index) order.  Same dict as ``grid_knn`` (no error bits)."""
    cand = np.asarray(cand, np.float32)
    B, M = cand.shape[:2]
    query = cand if query is None else np.asarray(query, np.float32)
    N = query.shape[1]
    nc = _counts(n_cand, B, M)
    nq = nc if query is cand else _counts(n_query, B, N)
    out = dict(idx=np.full((B, N, K), -1, np.int64), dist=np.full((B, N, K), np.nan, np.float32), count=np.full((B, N), -1, np.int32),
               written=np.zeros((B, N), bool))
    for b in range(B):
        n = int(nq[b])
        d2 = dist2(query[b, :n, :3], cand[b, :, :3])
        with np.errstate(invalid="ignore"):
            part = (np.arange(M) < nc[b])[None, :] & (d2 <= np.float32(max_d2))
        out["idx"][b, :n], out["dist"][b, :n], out["count"][b, :n] = _select(d2, part, K, M)
        out["written"][b, :n] = True
    return out
