"""CPU: tests/geometry_ref.py (the fp64 statements the GPU edge sweep of tests/test_geometry_edges_gpu.py is held to) against
the oracle's C restatement and the recorded vectors.  On lattice inputs the two must agree EXACTLY -- the oracle computes the
kernels' expanded float32 form, geometry_ref the fp64 difference form, and on the lattice both are exact -- and every lattice
case asserts that it really holds what it is there for (pairs on the radius, empty / short / full balls, ties at the third
neighbour), so that a change of seed cannot silently empty it."""
import numpy as np
import pytest

import geometry_ref as R
from conftest import golden
from oracle import geometry as G

B, N, S = 3, 2240, 37


def _clouds(seed=2240):
    rng = np.random.default_rng(seed)
    return R.lattice(rng, B, N), R.lattice(rng, B, S)


def test_lattice_is_the_documented_grid():
    xyz = R.lattice(np.random.default_rng(0), 2, 5000)
    assert xyz.dtype == np.float32 and xyz.shape == (2, 5000, 3)
    assert set(np.unique(xyz * 8).tolist()) == set(range(-8, 8))


def test_square_distance_is_exact_on_the_lattice():
    xyz, new = _clouds()
    d64 = R.square_distance64(new, xyz)
    d32 = G.square_distance(new, xyz)
    assert d32.dtype == np.float32 and (d32.astype(np.float64) == d64).all()
    assert (d64 == 0).any() and d64.max() > 8                    # coincident points and far corners are both in


# r, k, and what the case is there for: balls that are empty / short (0 < hits < k) / full (hits >= k)
BALL_CASES = [(1 / 16, 8, "empty short"), (1 / 8, 1, "empty full"), (1 / 8, 7, "empty short full"), (3 / 8, 65, "short full"),
              (3 / 8, 200, "short"), (1.0, N, "short"), (8.0, 128, "full")]


@pytest.mark.parametrize("r,k,kinds", BALL_CASES)
def test_query_ball_equals_the_oracle_on_the_lattice(r, k, kinds):
    xyz, new = _clouds()
    mine = R.query_ball64(r, k, xyz, new)
    assert mine.dtype == np.int64 and (mine == G.query_ball_point(r, k, xyz, new)).all()
    d = R.square_distance64(new, xyz)
    hits = (~(d > r * r)).sum(-1)
    if r in (1 / 8, 3 / 8, 1.0):                                 # (1/256 is no sum of three squares of eighths; 64 is out of reach)
        assert (d == r * r).sum() >= 1, "no pair exactly on the radius"
    have = {"empty": (hits == 0).any(), "short": ((hits > 0) & (hits < k)).any(), "full": (hits >= k).any()}
    for kind in kinds.split():
        assert have[kind], "the case holds no %s ball" % kind
    # the statement itself, slot by slot, on the first cloud
    for s in range(S):
        inside = [j for j in range(N) if not d[0, s, j] > r * r]
        want = (inside[:k] + [inside[0]] * k)[:k] if inside else [N] * k
        assert mine[0, s].tolist() == want


def test_boundary_pairs_are_kept():
    """d == r^2 is inside the ball (the reference drops d > r^2 only): among the lattice cases the radii 1/8, 3/8 and 1
    all see pairs exactly on the boundary, and they appear in the result."""
    xyz, new = _clouds()
    for r in (1 / 8, 3 / 8, 1.0):
        d = R.square_distance64(new, xyz)
        on = np.argwhere(d == r * r)
        assert len(on) >= 100, (r, len(on))
        idx = R.query_ball64(r, N, xyz, new)
        b, s, j = on[0]
        assert j in idx[b, s]


def test_query_ball_equals_the_recorded_edge_cases():
    """The recorded boundary clouds hold points whose FLOAT32 distance is float32(r^2) exactly and one ulp either side; the
    reference keeps the first two.  That is a statement about float32 rounding (r = 0.1 is no float32 and the squares are
    inexact), so the selection rule of geometry_ref is held to the record on the float32 distances and threshold the kernels
    see; in fp64 the middle point lies ~1e-16 outside r*r, and that one pair is all the plain fp64 statement may differ in."""
    g = golden("g2_ball.npz")
    for r in (0.1, 0.2, 0.4, 0.8):
        pre = "edge/r%g/" % r
        xyz, new, ref = g[pre + "xyz"], g[pre + "new_xyz"], g[pre + "idx"]
        d32 = G.square_distance(new, xyz)[0, 0]
        r2 = np.float32(r ** 2)
        assert (R.ball_from_distances(d32, r2, 4) == ref[0, 0]).all(), r
        on = np.flatnonzero(d32 == r2)
        assert on.tolist() == [1]                                # the pair on the float32 boundary
        d64 = R.square_distance64(new, xyz)[0, 0]
        keep = np.arange(xyz.shape[1]) != 1
        assert ((d64 > r * r) == (d32 > r2))[keep].all()
        assert (R.query_ball64(r, 4, xyz[:, keep], new) == R.ball_from_distances(d32[keep], r2, 4)).all()


def test_three_nn_equals_the_oracle_on_the_lattice():
    rng = np.random.default_rng(257)
    q, c = R.lattice(rng, 3, 257), R.lattice(rng, 3, 1025)
    idx, dist, w = R.three_nn64(q, c)
    oi, od = G.three_nn(q, c)
    assert idx.dtype == np.int64 and (idx == oi).all()
    assert (od.astype(np.float64) == dist).all()
    assert np.abs(G.three_weights(od) - w).max() <= 1.2e-7
    assert np.abs(w.sum(-1) - 1).max() <= 1e-15
    d = np.sort(R.square_distance64(q, c), -1)
    assert (d[..., 2] == d[..., 3]).mean() >= 0.10, "fewer than 10 % of the rows are tied at the third / fourth neighbour"
    assert (dist == 0).mean() >= 0.01, "no coincident neighbours"
    assert (np.diff(dist, axis=-1) >= 0).all()
    tied = dist[..., 0] == dist[..., 1]
    assert tied.any() and (idx[..., 0][tied] < idx[..., 1][tied]).all()      # ties go to the lower index


def test_three_nn_equals_the_recorded_case_c():
    g = golden("g4_interp.npz")
    idx, dist, w = R.three_nn64(g["c/xyz1"], g["c/xyz2"])
    oi, od = G.three_nn(g["c/xyz1"], g["c/xyz2"])
    assert (idx == oi).all()
    # continuous inputs: the recorded float32 distances carry the rounding of the expanded form (a few ulps of |q|^2 + |p|^2)
    scale = (g["c/xyz1"].astype(np.float64) ** 2).sum(-1).max() + (g["c/xyz2"].astype(np.float64) ** 2).sum(-1).max()
    assert np.abs(g["c/dist3"] - dist).max() <= 4 * 2.0 ** -24 * scale
