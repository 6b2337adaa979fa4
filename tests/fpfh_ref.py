"""The FPFH rule of include/pn2.h ("FPFH") in numpy: what pn2_spfh and pn2_fpfh must write, and the inputs the CPU and the GPU
tests share.

Every operation is the fp64 statement of the header, one rounding each (numpy never fuses), vectorised over the rows of a cloud
with the K slots in a Python loop, so sums run in ascending slot order.  ``spfh`` also says which rows hold a pair whose ``t``
lies within ``edge`` of a bin edge: only there may an ``atan2`` that differs from libm's by a few ulp move a count."""
import math

import numpy as np

ERR_EMPTY, ERR_NONFINITE = 1, 2
PI = 3.14159265358979323846
EDGE = 2.0 ** -30


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _bin(t):
    with np.errstate(invalid="ignore"):
        return np.where(t >= 1.0, np.where(t >= 10.0, 10, np.floor(np.where(np.isfinite(t), t, 0.0))), 0).astype(np.int64)


def _near_edge(t, edge, lo, hi):
    r = np.rint(t)
    return (np.abs(t - r) <= edge) & (r >= lo) & (r <= hi)


def geometric(points, idx, max_d2, n):
    """points [M, >=3] float32, idx [M,K] -> (ok [n,K] bool: the slot passes G1..G3, d2 [n,K] fp64, j [n,K] clipped, nonfinite [n,K]:
    the slot is in range and one of its two points is not finite)."""
    p = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    j = np.asarray(idx, np.int64)[:n]
    inr = (j >= 0) & (j < n)
    jj = np.where(inr, j, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        dp = p[jj] - p[:n, None, :]
        fin = np.isfinite(p[jj]).all(-1) & np.isfinite(p[:n, None, :]).all(-1)
        d2 = _dot(dp, dp)
        ok = inr & fin & (d2 > 0.0) & (d2 <= np.float64(np.float32(max_d2)))
    return ok, d2, jj, inr & ~fin, dp


def pair_features(dp, ni, nj):
    """dp, ni, nj [..., 3] fp64 -> (t1, t2, t3, y, vl): the three bin coordinates before the floor, atan2's first argument, |v|."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.sqrt(_dot(dp, dp))
        a1, a2 = _dot(ni, dp) / d, _dot(nj, dp) / d
        on_j = (np.abs(a1) < np.abs(a2))[..., None]
        ns, nt = np.where(on_j, nj, ni), np.where(on_j, ni, nj)
        dp = np.where(on_j, -dp, dp)
        f3 = np.where(on_j[..., 0], -a2, a1)
        v = _cross(dp, ns)
        vl = np.sqrt(_dot(v, v))
        v = v / vl[..., None]
        w = _cross(ns, v)
        f2 = _dot(v, nt)
        y = _dot(w, nt) + 0.0
        f1 = np.arctan2(y, _dot(ns, nt))
        t1 = 11.0 * (f1 + PI) / (2.0 * PI)
        t2 = 11.0 * (f2 + 1.0) * 0.5
        t3 = 11.0 * (f3 + 1.0) * 0.5
    return t1, t2, t3, y, vl


def spfh_cloud(points, normals, idx, max_d2=np.inf, n=None, edge=EDGE):
    """One cloud: points [M, >=3], normals [M, >=3] float32 (columns 0..2), idx [M,K] int64 -> (bytes uint8 [n,36], flagged bool [n],
    err)."""
    M = len(points)
    n = M if n is None else max(0, min(M, int(n)))
    K = np.asarray(idx).shape[1]
    ok, d2, jj, nonfin, dp = geometric(points, idx, max_d2, n)
    nr = np.asarray(normals, np.float32)[:, :3].astype(np.float64)
    out = np.zeros((n, 36), np.uint8)
    flagged = np.zeros(n, bool)
    err = ERR_NONFINITE if nonfin.any() else 0
    rows = np.arange(n)
    for s in range(K):
        ni, nj = nr[:n], nr[jj[:, s]]
        nfin = np.isfinite(ni).all(-1) & np.isfinite(nj).all(-1)
        if (ok[:, s] & ~nfin).any():
            err |= ERR_NONFINITE
        t1, t2, t3, y, vl = pair_features(dp[:, s], ni, nj)
        with np.errstate(invalid="ignore"):
            pair = ok[:, s] & nfin & ~(ni == 0).all(-1) & ~(nj == 0).all(-1) & (vl > 0.0)
        r = rows[pair]
        np.add.at(out, (r, _bin(t1)[pair]), 1)
        np.add.at(out, (r, 11 + _bin(t2)[pair]), 1)
        np.add.at(out, (r, 22 + _bin(t3)[pair]), 1)
        out[r, 33] += 1
        near = _near_edge(t2, edge, 1, 10) | _near_edge(t3, edge, 1, 10) | _near_edge(t1, edge, 1, 10) | \
            (_near_edge(t1, edge, 0, 11) & (y != 0.0))
        flagged |= pair & near
    if n and (out[:, 33] == 0).any():
        err |= ERR_EMPTY
    return out, flagged, err


def counts(spfh):
    """uint8 [..., 36] -> (counts int64 [..., 33], m int64 [...])."""
    a = np.asarray(spfh)
    return a[..., :33].astype(np.int64), a[..., 33].astype(np.int64)


def finish_cloud(points, idx, spfh, max_d2=np.inf, n=None, reduce=False):
    """One cloud: the FPFH rows of ``spfh`` uint8 [>=n,36] -> (fpfh float32 [n,33], the same before the last rounding fp64 [n,33],
    voters int64 [n], err).  ``reduce``: W and A by ``np.add.reduce`` over the slots instead of one slot after another (numpy's
    pairwise order: the restatement a test holds the loop to)."""
    M = len(points)
    n = M if n is None else max(0, min(M, int(n)))
    K = np.asarray(idx).shape[1]
    ok, d2, jj, nonfin, _ = geometric(points, idx, max_d2, n)
    c, m = counts(np.asarray(spfh)[:n])
    c, m = c.astype(np.float64), m.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(m[:, None] > 0, (100.0 * c) / m[:, None], 0.0)
        votes = ok & (m[jj] > 0)
        if reduce:
            W = np.add.reduce(np.where(votes, 1.0 / d2, 0.0), 1)
            A = np.add.reduce(np.where(votes[..., None], s[jj] / d2[..., None], 0.0), 1)
        else:
            W, A = np.zeros(n), np.zeros((n, 33))
            for k in range(K):
                W = W + np.where(votes[:, k], 1.0 / d2[:, k], 0.0)
                A = A + np.where(votes[:, k, None], s[jj[:, k]] / d2[:, k, None], 0.0)
        f = s + np.where(W[:, None] > 0, A / W[:, None], 0.0)
    err = (ERR_NONFINITE if nonfin.any() else 0) | (ERR_EMPTY if n and (m == 0).any() else 0)
    return f.astype(np.float32), f, votes.sum(1), err


def _batched(fn, B, n_points, M):
    ns = [M] * B if n_points is None else [max(0, min(M, int(v))) for v in n_points]
    return [fn(b, ns[b]) for b in range(B)], ns


def spfh(points, normals, idx, max_d2=np.inf, n_points=None, before=None, edge=EDGE):
    """points [B,M,ldp], normals [B,M,>=3] (the caller slices normal_col away), idx [B,M,K] -> (bytes uint8 [B,M,36], flagged
    [B,M], err); rows at and beyond n_points hold ``before`` (default: zeros)."""
    B, M = np.asarray(points).shape[:2]
    out = np.zeros((B, M, 36), np.uint8) if before is None else np.array(before, np.uint8)
    flagged, err = np.zeros((B, M), bool), 0
    res, ns = _batched(lambda b, n: spfh_cloud(points[b], normals[b], idx[b], max_d2, n, edge), B, n_points, M)
    for b, (o, f, e) in enumerate(res):
        out[b, :ns[b]], flagged[b, :ns[b]], err = o, f, err | e
    return out, flagged, err


def finish(points, idx, spfh_bytes, max_d2=np.inf, n_points=None, before=None):
    """The batched ``finish_cloud`` -> (fpfh float32 [B,M,33], voters [B,M], err)."""
    B, M = np.asarray(points).shape[:2]
    out = np.zeros((B, M, 33), np.float32) if before is None else np.array(before, np.float32)
    voters, err = np.zeros((B, M), np.int64), 0
    res, ns = _batched(lambda b, n: finish_cloud(points[b], idx[b], spfh_bytes[b], max_d2, n), B, n_points, M)
    for b, (f, _, v, e) in enumerate(res):
        out[b, :ns[b]], voters[b, :ns[b]], err = f, v, err | e
    return out, voters, err


# ----------------------------------------------------------------------------- shared inputs (read-only, made once)
def knn_self(points, k, n=None):
    """Brute-force self-search in fp64: idx int64 [M,k], ascending (d2, index); rows at and beyond n, and slots past n, hold M."""
    p = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    M = len(p)
    n = M if n is None else n
    idx = np.full((M, k), M, np.int64)
    if n:
        d = ((p[:n, None, :] - p[None, :n, :]) ** 2).sum(-1)
        order = np.lexsort((np.broadcast_to(np.arange(n), d.shape), d), axis=1)[:, :k]
        idx[:n, :order.shape[1]] = order
    return idx


_made = {}


def wavy_sheet(M=1024, seed=5):
    """(points [M,3], normals [M,3]) float32, read-only: z = 0.15 sin(1.3 x) cos(1.1 y) over [-2,2]^2 with its analytic unit
    normals (pointing to +z)."""
    key = ("sheet", M, seed)
    if key not in _made:
        rng = np.random.default_rng(seed)
        u, v = rng.uniform(-2, 2, M), rng.uniform(-2, 2, M)
        h = 0.15 * np.sin(1.3 * u) * np.cos(1.1 * v)
        hu, hv = 0.15 * 1.3 * np.cos(1.3 * u) * np.cos(1.1 * v), -0.15 * 1.1 * np.sin(1.3 * u) * np.sin(1.1 * v)
        nrm = np.stack([-hu, -hv, np.ones(M)], -1)
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        pts = np.stack([u, v, h], -1).astype(np.float32)
        nrm = nrm.astype(np.float32)
        pts.setflags(write=False)
        nrm.setflags(write=False)
        _made[key] = (pts, nrm)
    return _made[key]


DIRECTIONS = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0.6, 0, 0.8], [0, 0.6, -0.8], [0.6, 0.8, 0], [-0.8, 0, 0.6]], np.float32)


def lattice(seed=9):
    """(points [75,3], normals [75,3]) float32, read-only: a 5 x 5 x 3 lattice of pitch 0.25 with normals drawn from the eight fixed
    ``DIRECTIONS``: many exact ties of |a1| and |a2|, zero |v| and antiparallel normals."""
    key = ("lattice", seed)
    if key not in _made:
        g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
        pts = (0.25 * g).astype(np.float32)
        nrm = DIRECTIONS[np.random.default_rng(seed).integers(0, len(DIRECTIONS), len(pts))].copy()
        pts.setflags(write=False)
        nrm.setflags(write=False)
        _made[key] = (pts, nrm)
    return _made[key]


def plane_lattice():
    """(points [64,3], normals [64,3]): an 8 x 8 lattice of pitch 0.5 in z = 0 with normals +z."""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([0.5 * g, np.zeros((64, 1))], 1).astype(np.float32)
    return pts, np.tile(np.array([0, 0, 1], np.float32), (64, 1))
