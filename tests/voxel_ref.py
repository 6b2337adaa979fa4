"""numpy restatement of the voxel-grid rule (include/pn2.h, ``pn2_voxel_grid``), for the tests.

Per axis ``q = floor((float64(p) - origin) / voxel)`` in IEEE fp64; a row is valid iff ``-2**20 <= q < 2**20`` on all three axes
(compared in fp64: NaN and +-inf fail); the key packs the three biased 21-bit cells into 63 bits; rows with equal keys form a voxel,
its representative is its lowest row, and the representatives come in ascending row number --
``np.sort(np.unique(key, return_index=True)[1])``.
"""
import numpy as np

LIMIT = 1 << 20


def triple(v):
    a = np.asarray(v, np.float64).reshape(-1)
    return np.repeat(a, 3) if a.size == 1 else a.reshape(3)


def cells(points, origin, voxel):
    """``(q float64 [M, 3], valid bool [M])``."""
    p = np.asarray(points)[:, :3].astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.floor((p - triple(origin)[None, :]) / triple(voxel)[None, :])
        valid = ((q >= -float(LIMIT)) & (q < float(LIMIT))).all(1)
    return q, valid


def keys(points, origin, voxel):
    """``(key int64 [M] (0 where invalid), valid bool [M])``."""
    q, valid = cells(points, origin, voxel)
    c = np.where(valid[:, None], q, 0.0).astype(np.int64) + LIMIT
    return np.where(valid, (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], 0), valid


def voxel_grid(points, origin, voxel, labels=None):
    """The rule on one cloud ``[M, ld]`` float32.  Returns a dict: ``valid`` bool ``[M]``, ``key`` int64 ``[M]``; ``index`` int32
    (the representatives' rows, ascending), ``points`` (those rows, all ``ld`` columns), ``labels`` int32 (zeros without
    ``labels``), ``n_points`` int32 (valid rows per voxel), ``count``, and ``inverse`` int32 ``[M]`` (the rank of each row's voxel, -1
    for an invalid row)."""
    points = np.ascontiguousarray(points, np.float32)
    M = len(points)
    key, valid = keys(points, origin, voxel)
    rows = np.flatnonzero(valid)
    uniq, first, inv, pop = np.unique(key[rows], return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")                         # the voxels by their first (= lowest) row
    rank_of = np.empty(len(uniq), np.int64)
    rank_of[order] = np.arange(len(uniq))
    index = rows[first[order]].astype(np.int32)
    inverse = np.full(M, -1, np.int32)
    inverse[rows] = rank_of[np.asarray(inv).reshape(-1)]
    lab = np.zeros(len(index), np.int32) if labels is None else np.asarray(labels).astype(np.int32)[index]
    return {"valid": valid, "key": key, "index": index, "points": points[index], "labels": lab,
            "n_points": pop[order].astype(np.int32), "count": len(index), "inverse": inverse}


def brute_force(points, origin, voxel):
    """The O(M^2) restatement: ``(index, inverse, n_points)`` from pairwise comparisons of the fp64 cells, no keys and no sort."""
    q, valid = cells(points, origin, voxel)
    M = len(q)
    same = valid[:, None] & valid[None, :] & (q[:, None, :] == q[None, :, :]).all(2)
    index, inverse, n_points = [], np.full(M, -1, np.int32), []
    for i in range(M):
        if not valid[i]:
            continue
        mates = np.flatnonzero(same[i])
        if mates[0] == i:                                            # no earlier row in this cell: a representative
            index.append(i)
            n_points.append(len(mates))
    rank = {r: k for k, r in enumerate(index)}
    for i in range(M):
        if valid[i]:
            inverse[i] = rank[int(np.flatnonzero(same[i])[0])]
    return np.array(index, np.int32), inverse, np.array(n_points, np.int32)
