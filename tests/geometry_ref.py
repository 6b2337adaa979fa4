"""fp64 statements of the three query operations of csrc/geometry.hip -- pair distances, ball query, 3-NN with its
inverse-distance weights -- and the lattice inputs on which they are exact.  A test helper written in numpy from the
formulas of include/pn2.h and the docstrings of pointnet_util.py, for clarity, not speed.

THE LATTICE.  ``lattice`` draws every coordinate from {-8, ..., 7} / 8.  A product of two such numbers is a multiple of
1/64 below 1, a sum of three of them or of the squares of three differences a multiple of 1/64 below 16: each fits a
float32 with bits to spare.  So every product and every sum of both the kernels' expanded form |q|^2 + |p|^2 - 2 q.p
(with or without fused steps) and the difference form sum (q - p)^2 is exact in float32, the float32 distance IS the
fp64 distance, and a kernel must reproduce these statements bit for bit and index for index -- no tolerance band, no
pair left out near the radius, and nothing that leans on the reference sharing the kernel's formula.  The same holds
for coordinates that are whole numbers of eighths up to +-16 (the planted cases of tests/test_geometry_edges_gpu.py).
With 4096 lattice positions, clouds of a few thousand points hold many coincident points (d == 0), many pairs exactly
on a radius that is itself a multiple of 1/8 (d == r^2) and many ties among the nearest neighbours.
"""
import numpy as np


def lattice(rng, B, N):
    """[B, N, 3] float32 with every coordinate in {-8, ..., 7} / 8."""
    return (rng.integers(-8, 8, (B, N, 3)) / 8).astype(np.float32)


def square_distance64(src, dst):
    """src [B,S,3], dst [B,N,3] -> [B,S,N] fp64: sum over the three axes of (q - p)^2."""
    q = np.asarray(src, np.float64)[:, :, None, :]
    p = np.asarray(dst, np.float64)[:, None, :, :]
    out = np.zeros(q.shape[:2] + (p.shape[2],))
    for a in range(3):                                   # one axis at a time: no [B,S,N,3] temporary
        out += (q[..., a] - p[..., a]) ** 2
    return out


def ball_from_distances(d, r2, k):
    """One centre's row of distances d [N] -> int64 [k]: the ascending indices with not (d > r2), the first k of them, the
    remaining slots filled with the first hit; an empty ball is N in every slot."""
    hits = np.flatnonzero(~(d > r2))[:k]
    out = np.full(k, d.shape[0] if hits.size == 0 else hits[0], np.int64)
    out[:hits.size] = hits
    return out


def query_ball64(r, k, xyz, new_xyz):
    """xyz [B,N,3], new_xyz [B,S,3] -> int64 [B,S,k]: ``ball_from_distances`` of every centre's fp64 distances, r2 = r*r."""
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    out = np.empty((B, S, k), np.int64)
    for b in range(B):
        for s0 in range(0, S, 128):                      # (a slab of centres at a time keeps the distance matrix small)
            d = square_distance64(new_xyz[b:b + 1, s0:s0 + 128], xyz[b:b + 1])[0]
            for i in range(d.shape[0]):
                out[b, s0 + i] = ball_from_distances(d[i], r * r, k)
    return out


def three_nn64(xyz1, xyz2):
    """xyz1 [B,N,3] queries, xyz2 [B,S,3] candidates, S >= 3 -> (idx int64 [B,N,3], dist fp64 [B,N,3], weight fp64
    [B,N,3]): the first three of a STABLE argsort of the fp64 distances (ties go to the lower index), the distances
    themselves, and the weights 1 / max(d, 1e-10) normalised to sum 1."""
    d = square_distance64(xyz1, xyz2)
    idx = np.argsort(d, axis=-1, kind="stable")[..., :3]
    dist = np.take_along_axis(d, idx, -1)
    w = 1.0 / np.maximum(dist, 1e-10)
    return idx.astype(np.int64), dist, w / w.sum(-1, keepdims=True)
