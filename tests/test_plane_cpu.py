"""CPU: the plane rule's numpy restatement (tests/plane_ref.py) tested on its own -- the sampler, the exact-plane case, ties, the
collinear cloud, and the ground of the synthetic scan."""
import numpy as np
import pytest

import plane_ref as P
from pointnet12_amd import synthetic

COS15 = float(np.cos(np.radians(15.0)))


def test_sampler_stays_in_range_and_both_forms_agree():
    for n in (1, 2, 3, 2 ** 29):
        for seed, b in ((0, 0), (7, 3), (2 ** 63 + 12345, 65534)):
            rows = P.sample_rows(seed, b, 2048, n)
            assert rows.min() >= 0 and rows.max() < n
            for h in (0, 1, 255, 2047):
                assert [P.sample(seed, b, h, j, n) for j in range(3)] == rows[h].tolist()
    assert (P.sample_rows(5, 0, 64, 1) == 0).all()
    assert set(P.sample_rows(5, 0, 512, 2).ravel().tolist()) == {0, 1}
    assert len(set(map(tuple, P.sample_rows(0, 0, 64, 1000).tolist()))) == 64 and not np.array_equal(P.sample_rows(0, 0, 64, 1000), P.sample_rows(1, 0, 64, 1000))
    assert not np.array_equal(P.sample_rows(0, 0, 64, 1000), P.sample_rows(0, 1, 64, 1000))


def test_sampler_is_uniform():
    """60 000 draws into 1 000 rows: chi-square per degree of freedom in [0.8, 1.2] (its standard deviation at 999 degrees is 0.045)."""
    rows = P.sample_rows(0, 0, 20000, 1000).ravel()
    hist = np.bincount(rows, minlength=1000)
    chi = ((hist - 60.0) ** 2 / 60.0).sum() / 999
    print("chi-square per degree of freedom: %.3f" % chi)
    assert 0.8 <= chi <= 1.2


def lattice_plane(rng, n_in, n_out):
    """n_in rows of the lattice plane x + 2 y + 2 z = 3 (coordinates multiples of 1/8, exact) and n_out lattice rows at least 1/8
    off it along the normal, shuffled."""
    xy = rng.integers(-16, 16, (n_in, 2)) / 8
    inl = np.stack([3.0 - 2 * xy[:, 0] - 2 * xy[:, 1], xy[:, 0], xy[:, 1]], 1)
    out = rng.integers(-16, 16, (4 * n_out, 3)) / 8
    out = out[np.abs(out @ [1.0, 2.0, 2.0] - 3.0) >= 0.375][:n_out]
    assert len(out) == n_out
    pts = np.concatenate([inl, out]).astype(np.float32)
    order = rng.permutation(len(pts))
    return pts[order], np.isin(order, np.arange(n_in))


def test_exact_lattice_plane_with_outliers():
    pts, planted = lattice_plane(np.random.default_rng(1), 300, 200)
    r = P.fit_plane(pts[None], 2.0 ** -10, H=64, refine=2)
    want = np.array([1.0, 2.0, 2.0, -3.0]) / 3.0
    assert r["status"][0] == 0 and r["err"] == 0
    assert np.abs(r["plane0"][0] - want).max() <= 1e-12 and np.abs(r["plane"][0] - want).max() <= 1e-12
    assert r["best_count"][0] == r["count"][0] == 300 and np.array_equal(r["inlier"][0], planted)
    assert r["rmse"][0] <= 1e-7 and np.abs(r["dist"][0][planted]).max() <= 1e-6
    assert (np.abs(r["dist"][0][~planted]) >= 0.124).all()


def test_ties_go_to_the_lowest_hypothesis():
    pts, _ = lattice_plane(np.random.default_rng(2), 400, 100)
    r = P.ransac(pts[None], 2.0 ** -10, 256)
    counts = r["hyp_count"][0]
    best = counts.max()
    assert best == 400 and (counts == best).sum() > 1                  # several hypotheses found the plane: the tie is real
    assert r["best_h"][0] == np.flatnonzero(counts == best)[0] and r["best_count"][0] == best
    assert np.array_equal(r["plane"][0], r["hyp"][0, r["best_h"][0]])


def test_collinear_cloud_and_short_clouds_give_none():
    t = np.arange(64, dtype=np.float32)
    line = np.stack([t, 2 * t, -t], 1)[None]
    r = P.fit_plane(line, 0.5, H=64)
    assert r["status"][0] == P.NONE and r["err"] == P.ERR_NONE and (r["plane"][0] == 0).all() and r["best_h"][0] == -1
    assert (r["hyp_count"][0] == -1).all() and r["count"][0] == -1 and np.isnan(r["dist"][0]).all()
    pts, _ = lattice_plane(np.random.default_rng(3), 50, 10)
    for n in (0, 2):
        r = P.fit_plane(pts[None], 0.5, H=64, n_points=[n])
        assert r["status"][0] == P.NONE and r["best_h"][0] == -1


def test_angle_limit_and_flip():
    ax = P.unit_axis((0, 0, 2.0))
    assert np.array_equal(ax, [0, 0, 1.0])
    n = np.array([[0.0, 0.0, -1.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])
    assert np.array_equal(P.flip(n, ax), [[0, 0, 1.0], [0, 1.0, 0], [1.0, 0, 0], [0, 1.0, 0], [0.6, 0, 0.8]])
    # a wall x = 1 (dominant) and a floor z = 0: the floor is found only with the angle limit
    rng = np.random.default_rng(4)
    wall = np.stack([np.ones(600), rng.integers(-16, 16, 600) / 8, rng.integers(0, 32, 600) / 8], 1)
    floor = np.stack([rng.integers(-16, 16, 200) / 8, rng.integers(-16, 16, 200) / 8, np.zeros(200)], 1)
    pts = np.concatenate([wall, floor]).astype(np.float32)[rng.permutation(800)][None]
    free, held = P.fit_plane(pts, 0.01, H=128), P.fit_plane(pts, 0.01, H=128, cos_max=COS15)
    assert np.abs(free["plane"][0] - [1.0, 0, 0, -1.0]).max() <= 1e-12 and free["count"][0] >= 600
    assert np.abs(held["plane"][0] - [0, 0, 1.0, 0]).max() <= 1e-12 and 200 <= held["count"][0] < 300
    assert (held["hyp_count"][0] >= 0).sum() < (free["hyp_count"][0] >= 0).sum()


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("n,H", [(2048, 64), (20000, 256)])
def test_the_plane_of_a_synthetic_scan_is_the_ground(s, n, H):
    """The synthetic ground is a shallow cone (z = -1.73 cos phi), so the answer is not d = 1.73.  This restatement gives tilt
    0.37 - 0.54 degrees, d 1.593 - 1.612, rmse 0.033 - 0.038 and 66 - 72 % inliers on these six cases; the bounds (2 degrees, 1.5 < d < 1.7) were set before it ran."""
    pts = synthetic.kitti_scan(synthetic.SEED_BASE + s, n)[None, :, :3]
    r = P.fit_plane(pts, 0.1, H=H, cos_max=COS15, refine=2)
    tilt, d = float(P.tilt_degrees(r["plane"][0])), float(r["plane"][0, 3])
    print("s = %d, n = %d, H = %d: tilt %.3f deg, d %.4f, rmse %.4f, inliers %.1f %%" % (s, n, H, tilt, d, r["rmse"][0], 100.0 * r["count"][0] / n))
    assert r["status"][0] == 0 and tilt < 2.0 and 1.5 < d < 1.7
