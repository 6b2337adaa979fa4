"""GPU: pn2_plane_ransac / pn2_plane_refit / pn2_plane_classify against tests/plane_ref.py at the C ABI, and pointnet12_amd.plane on top.

The bounds, stated before any run:
  * every hypothesis count, best_h, best_count, status, the error bits, assign and the inlier sets EQUAL the reference's;
  * the selected plane before any refit equals the reference's hypothesis BIT FOR BIT (separately rounded fp64 on both sides);
  * the ten sums are the reference's terms in another order: |difference| <= count * 2^-52 * sum |term| (ICP's bound);
  * the refit plane against the header's finish (plane_ref.refit_finish) run on the DEVICE's own sums and plane: the same correctly
    rounded operations on both sides, held to 2^-48 (16 ulps of a unit normal: room for a square root that is not correctly rounded);
  * the refit plane against the reference's own: the covariance moves by at most dC = 4 * 2^-52 * (A_qq + 2 |m| A_q) (the sums
    bound divided by count, A = the largest sum of magnitudes), the eigenvector of l0 by at most dC / (l1 - l0) to first order;
    tol_n = 8 * dC / (l1 - l0) + 2^-48 and tol_d = tol_n * |s + m|_1 + 2^-52 * A_q + 2^-48;
  * dist equals the header's residual at the DEVICE's own plane in bits."""
import ctypes

import numpy as np
import pytest
import torch

import plane_ref as P
from pointnet12_amd import _lib, plane, synthetic, voxel

pytestmark = pytest.mark.gpu

F64_FILL, I64_FILL, I32_FILL, F32_FILL = -123.25, -77, -55, -9.5      # what outputs hold before a call: what a call must not touch keeps it
THR = 0.03
worst = {"sums": 0.0, "finish": 0.0, "plane": 0.0}


def cu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def triple(v):
    return (ctypes.c_double * 3)(*np.asarray(v, np.float64))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Cloud:
    """Clouds on the device with every output prefilled, and the three entry points as methods that return the code."""

    def __init__(self, dev, pts, H, n_points=None, assign=None, axis=(0, 0, 1), cos_max=0.0, threshold=THR, seed=0, fill=0xA5):
        lib = _lib.load()
        self.dev, self.pts_np, self.H, self.n_np, self.axis_np, self.cos_max, self.threshold, self.seed = dev, pts, H, n_points, axis, cos_max, threshold, seed
        self.B, self.N, self.ld = pts.shape
        self.axis = triple(axis)
        self.pts = cu(pts, dev)
        self.n_points = None if n_points is None else cu(np.asarray(n_points, np.int64), dev)
        self.assign = None if assign is None else cu(assign, dev)
        self.work = torch.full((lib.pn2_plane_workspace_bytes(self.B, self.N, H),), fill, device=dev, dtype=torch.uint8)       # (it may hold anything)
        B, N = self.B, self.N
        f = lambda shape, v, dt: torch.full(shape, v, device=dev, dtype=dt)
        self.out = dict(plane=f((B, 4), F64_FILL, torch.float64), hyp_count=f((B, H), I32_FILL, torch.int32), best_h=f((B,), I32_FILL, torch.int32),
                        best_count=f((B,), I64_FILL, torch.int64), status=f((B,), I32_FILL, torch.int32), err=f((1,), 0, torch.int32),
                        rmse=f((B,), F64_FILL, torch.float64), sums=f((B, 10), F64_FILL, torch.float64), dist=f((B, N), F32_FILL, torch.float32),
                        count=f((B,), I64_FILL, torch.int64))

    def args(self, over):
        p, o = _lib.ptr, self.out
        a = dict(pts=p(self.pts), ld=self.ld, B=self.B, N=self.N, n_points=p(self.n_points), assign=p(self.assign), H=self.H, seed=self.seed,
                 axis=ctypes.addressof(self.axis), cos_max=self.cos_max, threshold=self.threshold, plane=p(o["plane"]), hyp_count=p(o["hyp_count"]),
                 best_h=p(o["best_h"]), best_count=p(o["best_count"]), status=p(o["status"]), err=p(o["err"]), work=p(self.work),
                 rmse=p(o["rmse"]), sums=p(o["sums"]), dist=p(o["dist"]), count=p(o["count"]), plane_id=0, min_inliers=0)
        a.update(over)
        return a

    def ransac(self, **over):
        a = self.args(over)
        return _lib.load().pn2_plane_ransac(a["pts"], a["ld"], a["B"], a["N"], a["n_points"], a["assign"], a["H"], a["seed"], a["axis"], a["cos_max"],
                                            a["threshold"], a["plane"], a["hyp_count"], a["best_h"], a["best_count"], a["status"], a["err"],
                                            a["work"], _lib.stream())

    def refit(self, **over):
        a = self.args(over)
        return _lib.load().pn2_plane_refit(a["pts"], a["ld"], a["B"], a["N"], a["n_points"], a["assign"], a["axis"], a["threshold"], a["plane"],
                                           a["rmse"], a["sums"], a["status"], a["work"], _lib.stream())

    def classify(self, **over):
        a = self.args(over)
        return _lib.load().pn2_plane_classify(a["pts"], a["ld"], a["B"], a["N"], a["n_points"], a["assign"], a["plane_id"], a["min_inliers"],
                                              a["threshold"], a["plane"], a["status"], a["dist"], a["count"], a["work"], _lib.stream())

    def host(self):
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        got["assign"] = None if self.assign is None else self.assign.cpu().numpy()
        return got

    def counts(self):
        return np.full(self.B, self.N, np.int64) if self.n_np is None else np.clip(np.asarray(self.n_np, np.int64), 0, self.N)


_cases = {}


def lattice_case(N, ld, seed=None):
    """B = 3 lattice clouds (coordinates multiples of 1/8: exactly representable, so ties are real) with the device-side counts
    (N, 2, 0), drawn from ``seed`` (1000 N + ld unless given).  About half the rows lie on the lattice plane z = -1/4; every seventh
    row repeats row 0 (degenerate triples); from N = 63 on a NaN row, an inf row and rows that take no part (assign >= 0).  Host
    arrays, read-only, made once."""
    key = (N, ld, seed)
    if key not in _cases:
        rng = np.random.default_rng(1000 * N + ld if seed is None else seed)
        B = 3
        pts = np.zeros((B, N, ld), np.float32)
        pts[..., :3] = rng.integers(-8, 8, (B, N, 3)) / 8
        pts[..., 3:] = rng.random((B, N, ld - 3))                    # (not coordinates)
        pts[:, rng.random(N) < 0.5, 2] = -0.25
        pts[:, 1::7, :3] = pts[:, :1, :3]
        assign = None
        if N >= 63:
            pts[0, 5, 1], pts[0, 9, 0] = np.nan, np.inf
            assign = np.where(rng.random((B, N)) < 0.1, 5, -1).astype(np.int32)
            assign[0, 5] = assign[0, 9] = -1                        # the rows that are not finite take part: the error bit
            assign.setflags(write=False)
        pts.setflags(write=False)
        _cases[key] = (pts, np.int64([N, 2, 0]), assign)
    return _cases[key]


def check_refit_round(c, got, plane_in, status_in):
    """One pn2_plane_refit of clouds whose plane was ``plane_in`` (the device's): the module docstring's three bounds."""
    ns = c.counts()
    for b in range(c.B):
        if status_in[b] & P.NONE:
            assert (got["sums"][b] == F64_FILL).all() and got["rmse"][b] == F64_FILL and np.array_equal(bits(got["plane"][b]), bits(plane_in[b]))
            continue
        a_b = None if c.assign is None else c.assign_before[b]
        inl = P.inliers(c.pts_np[b], int(ns[b]), a_b, plane_in[b], c.threshold)
        sums, abs_sums = P.refit_sums(c.pts_np[b], inl, plane_in[b])
        count = float(inl.sum())
        assert got["sums"][b, 0] == count
        diff, bound = np.abs(got["sums"][b] - sums), count * 2.0 ** -52 * abs_sums
        worst["sums"] = max(worst["sums"], float((diff / np.maximum(bound, 1e-300)).max()))
        assert (diff <= bound).all()
        want, rmse, degenerate = P.refit_finish(got["sums"][b], plane_in[b], c.axis_np)
        assert bool(got["status"][b] & P.DEGENERATE) == degenerate or bool(status_in[b] & P.DEGENERATE)
        if degenerate:
            assert np.array_equal(bits(got["plane"][b]), bits(plane_in[b]))
            continue
        e = np.abs(got["plane"][b] - want).max()
        worst["finish"] = max(worst["finish"], float(e / 2.0 ** -48))
        assert e <= 2.0 ** -48 and abs(got["rmse"][b] - rmse) <= 2.0 ** -48 * max(rmse, 2.0 ** -24)
        ref_plane, _, ref_deg = P.refit_finish(sums, plane_in[b], c.axis_np)
        if ref_deg:
            continue
        m = sums[1:4] / count
        C6 = sums[4:] / count - np.array([m[0] * m[0], m[0] * m[1], m[0] * m[2], m[1] * m[1], m[1] * m[2], m[2] * m[2]])
        l0, l1, _, _ = P.sym_eig3(C6)
        A_q, A_qq = abs_sums[1:4].max(), abs_sums[4:].max()
        dC = 4.0 * 2.0 ** -52 * (A_qq + 2.0 * np.abs(m).max() * A_q)
        tol_n = 8.0 * dC / max(l1 - l0, 1e-300) + 2.0 ** -48
        reach = np.abs(-plane_in[b][3] * plane_in[b][:3] + m).sum()
        tol_d = tol_n * reach + 2.0 ** -52 * A_q + 2.0 ** -48
        e_n, e_d = np.abs(got["plane"][b, :3] - ref_plane[:3]).max(), abs(got["plane"][b, 3] - ref_plane[3])
        worst["plane"] = max(worst["plane"], float(e_n / tol_n), float(e_d / tol_d))
        assert e_n <= tol_n and e_d <= tol_d


def check_classify(c, got, plane_in, status_in, plane_id=0, min_inliers=0):
    ns = c.counts()
    for b in range(c.B):
        a_b = None if c.assign is None else c.assign_before[b]
        if status_in[b] & P.NONE:
            assert (got["dist"][b] == F32_FILL).all() and got["count"][b] == I64_FILL
            assert c.assign is None or np.array_equal(got["assign"][b], a_b)
            continue
        n = int(ns[b])
        dist, inl = P.classify(c.pts_np[b], n, a_b, plane_in[b], c.threshold)
        assert np.array_equal(got["dist"][b, :n].view(np.uint32), dist[:n].view(np.uint32)) and (got["dist"][b, n:] == F32_FILL).all()
        assert got["count"][b] == inl.sum()
        small = inl.sum() < min_inliers
        assert bool(got["status"][b] & P.SMALL) == small
        if c.assign is not None:
            want = a_b.copy()
            if not small:
                want[inl] = plane_id
            assert np.array_equal(got["assign"][b], want)


def run_pipeline(c, refine=2):
    """ransac, ``refine`` refits, classify at the C ABI, every stage checked against the reference at the device's own state, and the
    end against plane_ref.fit_plane as a whole (counts, status, assign, the inlier sets)."""
    c.assign_before = None if c.assign is None else c.assign.cpu().numpy().copy()
    ref_assign = None if c.assign is None else c.assign_before.copy()
    ref = P.fit_plane(c.pts_np, c.threshold, c.H, c.seed, c.axis_np, c.cos_max, refine, c.n_np, ref_assign)
    assert c.ransac() == 0
    got = c.host()
    assert np.array_equal(got["hyp_count"], ref["hyp_count"]) and np.array_equal(got["best_h"], ref["best_h"])
    assert np.array_equal(got["best_count"], ref["best_count"]) and int(got["err"][0]) == ref["err"]
    assert np.array_equal(got["status"] & P.NONE, ref["status"] & P.NONE)
    assert np.array_equal(bits(got["plane"]), bits(ref["plane0"]))
    for _ in range(refine):
        plane_in, status_in = got["plane"].copy(), got["status"].copy()
        assert c.refit() == 0
        got = c.host()
        check_refit_round(c, got, plane_in, status_in)
    plane_in, status_in = got["plane"].copy(), got["status"].copy()
    assert c.classify() == 0
    got = c.host()
    check_classify(c, got, plane_in, status_in)
    assert np.array_equal(got["status"], ref["status"])
    live = (ref["status"] & P.NONE) == 0
    assert np.array_equal(got["count"][live], ref["count"][live])
    if c.assign is not None:
        assert np.array_equal(got["assign"], ref_assign)
    for b in np.flatnonzero(live):
        n = int(c.counts()[b])
        a_b = None if c.assign is None else c.assign_before[b]
        assert np.array_equal(P.inliers(c.pts_np[b], n, a_b, got["plane"][b], c.threshold), ref["inlier"][b])
    return got, ref


@pytest.mark.parametrize("ld", [3, 4, 6])
@pytest.mark.parametrize("N", [3, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_pipeline_equals_the_reference(dev, N, ld):
    pts, n_points, assign = lattice_case(N, ld)
    for H in (1, 63, 64, 65, 256, 257):
        c = Cloud(dev, pts, H, n_points, assign, seed=N + H)
        got, ref = run_pipeline(c)
        assert got["status"][1] == got["status"][2] == P.NONE and (got["best_h"][1:] == -1).all() and (got["plane"][1:] == 0).all()
        assert int(got["err"][0]) & P.ERR_NONE
        if N >= 63:
            assert int(got["err"][0]) & P.ERR_NONFINITE
            if got["status"][0] == 0:
                assert np.isnan(got["dist"][0, 5]) and np.isnan(got["dist"][0, 9]) and got["assign"][0, 5] == got["assign"][0, 9] == -1
        if N >= 1023 and H >= 63:
            assert got["status"][0] == 0 and (ref["hyp_count"][0] == -1).any()        # the repeated rows made degenerate triples
        if N >= 1023 and H >= 256:                                  # (0.09 of the hypotheses lie in the planted plane: 256 of them do not all miss it)
            assert np.array_equal(got["plane"][0], [0, 0, 1.0, 0.25]) and got["count"][0] > N // 3         # the planted plane, exactly
    print("worst ratios to the bounds so far: %r" % worst)


# Past the first trip of the two loops over row tiles: the finish kernel's (thread (k, c) adds word k of tiles c, c + 8, c + 16, ...) at
# 9 and 17 tiles, the write kernel's (k += 256 over the tile counts) at 257 tiles, N = 262 145 being the smallest such N.  Counts: a
# cloud that ends exactly on a tile boundary with whole tiles of the launch beyond it, and (9, 17 tiles) one that ends inside a tile.
# Both seeds are chosen on the reference alone: the sampler's so that plane_ref.fit_plane gives status 0 for every cloud, the cloud's so
# that the LAST row of cloud 0 -- a tile of its own at N = 1024 t + 1 -- is an inlier, else that tile's partial and count would be zero
# and the last trip of either loop invisible (tests/test_tile_seams_cpu.py asserts it).
SEAM_CASES = {8193: ((8193, 8192, 5000), 65, 2, 0), 16385: ((16385, 8192, 9000), 65, 4, 0), 262145: ((262145, 262144), 64, 5, 0)}  # N: counts, H, seeds


def seam_case(N):
    """-> (pts, counts, assign, H, seed): ``lattice_case(N, 3)``'s clouds (the first two at 262 145 rows) with the counts above."""
    counts, H, cloud_seed, seed = SEAM_CASES[N]
    pts, _, assign = lattice_case(N, 3, cloud_seed)
    return pts[:len(counts)], np.int64(counts), assign[:len(counts)], H, seed


@pytest.mark.parametrize("N", sorted(SEAM_CASES))
def test_pipeline_past_the_first_trip_over_the_tiles(dev, N):
    """The workspace holds 0xFF bytes (NaN as a double, -1 as an integer): a word that is read and was not written poisons the result."""
    pts, counts, assign, H, seed = seam_case(N)
    c = Cloud(dev, pts, H, counts, assign, seed=seed, fill=0xFF)
    got, ref = run_pipeline(c)
    assert (ref["status"] == 0).all() and (ref["count"] > counts // 4).all() and ref["inlier"][0, N - 1]       # (the input's conditions)
    print("worst ratios to the bounds so far: %r" % worst)


def test_three_full_clouds_with_different_counts(dev):
    pts, _, assign = lattice_case(1025, 4)
    for n_points in ([1024, 1025, 513], None):
        c = Cloud(dev, pts, 65, n_points, assign, seed=3)
        got, ref = run_pipeline(c)
        assert (got["status"] == 0).all() and len(set(got["best_h"].tolist())) > 1             # b enters the sampler
    # an oblique axis and an angle limit, without assign
    c = Cloud(dev, pts, 257, None, None, axis=(0.5, -0.25, 2.0), cos_max=float(np.cos(np.radians(20.0))), seed=11)
    got, ref = run_pipeline(c)
    assert (got["status"] == 0).all() and (ref["hyp_count"] == -1).sum() > 3 * 64


def test_refusals_leave_every_output_untouched(dev):
    pts, n_points, assign = lattice_case(65, 4)
    c = Cloud(dev, pts, 64, n_points, assign)
    zero, nan_axis = triple((0, 0, 0)), triple((0, np.nan, 1))
    odd = _lib.ptr(c.work) + 8
    common = [dict(pts=None), dict(plane=None), dict(status=None), dict(work=None), dict(work=odd), dict(B=0), dict(B=65536), dict(N=0), dict(ld=2),
              dict(ld=17), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf"))]
    axes = [dict(axis=None), dict(axis=ctypes.addressof(zero)), dict(axis=ctypes.addressof(nan_axis))]
    for over in common + axes + [dict(best_h=None), dict(best_count=None), dict(H=0), dict(H=65537), dict(cos_max=float("nan"))]:
        assert c.ransac(**over) == -1, over
    for over in common + axes + [dict(rmse=None), dict(sums=None)]:
        assert c.refit(**over) == -1, over
    for over in common + [dict(count=None), dict(plane_id=-1)]:
        assert c.classify(**over) == -1, over
    lib = _lib.load()
    assert lib.pn2_plane_workspace_bytes(0, 5, 4) == -1 and lib.pn2_plane_workspace_bytes(1, 0, 4) == -1
    assert lib.pn2_plane_workspace_bytes(1, 5, 0) == -1 and lib.pn2_plane_workspace_bytes(1, 5, 65537) == -1
    assert lib.pn2_plane_workspace_bytes(1, 5, 65536) > 0 and lib.pn2_plane_workspace_bytes(2, 1025, 256) % 16 == 0
    got = c.host()
    assert (got["plane"] == F64_FILL).all() and (got["hyp_count"] == I32_FILL).all() and (got["best_h"] == I32_FILL).all()
    assert (got["best_count"] == I64_FILL).all() and (got["status"] == I32_FILL).all() and got["err"][0] == 0 and (got["rmse"] == F64_FILL).all()
    assert (got["sums"] == F64_FILL).all() and (got["dist"] == F32_FILL).all() and (got["count"] == I64_FILL).all()
    assert np.array_equal(got["assign"], assign)
    # optional pointers: no hyp_count, no err, no dist, no assign
    c2 = Cloud(dev, pts, 64, n_points, None)
    assert c2.ransac(hyp_count=None, err=None) == 0 and c2.refit() == 0 and c2.classify(dist=None) == 0
    got2 = c2.host()
    assert (got2["hyp_count"] == I32_FILL).all() and (got2["dist"] == F32_FILL).all() and got2["status"][0] == 0 and got2["count"][0] > 3


def wall_and_floor(rng):
    """A dominant wall x = 1 (600 rows), a floor z = 0 (200 rows) and 100 scattered rows, lattice coordinates, shuffled."""
    wall = np.stack([np.ones(600), rng.integers(-16, 16, 600) / 8, rng.integers(1, 32, 600) / 8], 1)
    floor = np.stack([rng.integers(-16, 8, 200) / 8, rng.integers(-16, 16, 200) / 8, np.zeros(200)], 1)
    rest = np.stack([rng.integers(-16, 8, 100) / 8 - 1 / 16, rng.integers(-16, 16, 100) / 8, rng.integers(1, 32, 100) / 8 + 1 / 16], 1)
    return np.concatenate([wall, floor, rest]).astype(np.float32)[rng.permutation(900)]


def test_wall_with_and_without_the_angle_limit(dev):
    pts = wall_and_floor(np.random.default_rng(5))
    d = cu(pts, dev)
    free = plane.fit_plane(d, 0.01, iterations=128)
    held = plane.fit_plane(d, 0.01, iterations=128, max_angle=15.0)
    assert free.plane.shape == (4,) and free.dist.shape == (900,) and free.count.dim() == 0
    ref_free = P.fit_plane(pts[None], 0.01, 128)
    ref_held = P.fit_plane(pts[None], 0.01, 128, cos_max=plane._cos_max(15.0))
    for got, ref, want, count in ((free, ref_free, [1.0, 0, 0, -1.0], 600), (held, ref_held, [0, 0, 1.0, 0], 200)):
        assert int(got.best_h) == ref["best_h"][0] and int(got.count) == ref["count"][0] == count and int(got.status) == 0
        assert np.abs(got.plane.cpu().numpy() - want).max() <= 1e-12 and float(got.rmse) <= 1e-7
        assert np.array_equal(np.abs(got.dist.cpu().numpy()) <= 0.01, ref["inlier"][0])
    assert np.array_equal(plane.height_above(d, held.plane).cpu().numpy().view(np.uint32), held.dist.cpu().numpy().view(np.uint32))
    with pytest.raises(_lib.Pn2Error):
        plane.fit_plane(torch.from_numpy(pts), 0.01)


def test_segment_planes_peels_in_order_of_size(dev):
    pts = wall_and_floor(np.random.default_rng(6))
    d = cu(pts, dev)
    seg = plane.segment_planes(d, 0.01, max_planes=3, min_inliers=150, iterations=1024)
    planes, counts, assign, status = (t.cpu().numpy() for t in seg)
    assert planes.shape == (3, 4) and counts.shape == (3,) and assign.shape == (900,) and status.shape == (3,)
    assert np.abs(planes[0] - [1.0, 0, 0, -1.0]).max() <= 1e-12 and np.abs(planes[1] - [0, 0, 1.0, 0]).max() <= 1e-12
    assert counts[0] == 600 and counts[1] == 200 and counts[2] < 150
    # (hypotheses are drawn among ALL rows and one that names a taken row is lost: 1 in 27 survives the wall, hence 1024 of them)
    assert status[0] == status[1] == 0 and status[2] & (P.SMALL | P.NONE)       # min_inliers stops the third: assign is left alone
    assert np.array_equal(assign == 0, pts[:, 0] == 1.0) and np.array_equal(assign == 1, (pts[:, 2] == 0.0) & (pts[:, 0] != 1.0))
    assert (assign[(pts[:, 0] != 1.0) & (pts[:, 2] != 0.0)] == -1).all() and set(assign.tolist()) == {-1, 0, 1}
    # the same through the reference, plane by plane on one assign
    ref_assign = np.full((1, 900), -1, np.int32)
    for k in range(3):
        r = P.fit_plane(pts[None], 0.01, 1024, seed=k, assign=ref_assign, plane_id=k, min_inliers=150)
        assert r["status"][0] == status[k] and (status[k] & P.NONE or r["count"][0] == counts[k])
    assert np.array_equal(ref_assign[0], assign)


def scan_batch(seeds, n):
    return np.stack([synthetic.kitti_scan(synthetic.SEED_BASE + s, n) for s in seeds])


def fit_bytes(res):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in res]


def test_scan_ground_equals_the_reference_and_two_runs_are_byte_identical(dev):
    pts = scan_batch((1, 2), 20000)                                 # [2, 20000, 4]: read where it lies
    d = cu(pts, dev)
    buf = plane.buffers(20000, 2, 256, device=dev)
    runs = []
    for _ in range(2):
        buf.dist.fill_(F32_FILL)
        res = plane.fit_plane(d, 0.1, iterations=256, max_angle=15.0, buffers=buf)
        runs.append(fit_bytes(res) + fit_bytes([buf.sums, buf.hyp_count, buf.best_count]))
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b))
    pl, count, rmse, dist, best_h, status = runs[0][:6]
    ref = P.fit_plane(pts, 0.1, 256, cos_max=plane._cos_max(15.0))
    assert np.array_equal(runs[0][7], ref["hyp_count"]) and np.array_equal(best_h, ref["best_h"]) and np.array_equal(runs[0][8], ref["best_count"])
    assert (status == 0).all() and np.array_equal(count, ref["count"]) and buf.error_flag.item() == 0
    for b in range(2):
        assert np.array_equal(P.inliers(pts[b], 20000, None, pl[b], 0.1), ref["inlier"][b])
    # The module docstring's bound at this size: dC <= 4 * 2^-52 * A_qq is about 1e-8 (14 000 inliers within 80 m), the gap l1 - l0
    # hundreds of m^2, the reach 80 m: below 1e-7 a round for n and for d; 1e-6 holds the two rounds with room.
    assert np.abs(pl - ref["plane"]).max() <= 1e-6 and np.abs(rmse - ref["rmse"]).max() <= 1e-6
    for b in range(2):
        tilt = float(P.tilt_degrees(pl[b]))
        print("cloud %d: tilt %.3f deg, d %.4f, rmse %.4f, %d inliers" % (b, tilt, pl[b, 3], rmse[b], count[b]))
        assert tilt < 2.0 and 1.5 < pl[b, 3] < 1.7


def test_graph_replay_on_new_points_counts_and_cleared_assign_equals_eager(dev):
    B, N, H = 2, 4096, 128
    cases = [(scan_batch((10 * k + 1, 10 * k + 2), N), np.int64([N - 300 * k, N // (k + 1)])) for k in range(3)]
    pts = torch.zeros(B, N, 4, device=dev)
    n_points = torch.zeros(B, device=dev, dtype=torch.int64)
    assign, eager_assign = torch.zeros(B, N, device=dev, dtype=torch.int32), torch.zeros(B, N, device=dev, dtype=torch.int32)
    buf, eager_buf = plane.buffers(N, B, H, device=dev), plane.buffers(N, B, H, device=dev)

    def run(b, a):
        return plane.fit_plane(pts, 0.1, iterations=H, seed=4, max_angle=15.0, n_points=n_points, assign=a, plane_id=3, min_inliers=10, buffers=b)

    def load(case):
        pts.copy_(cu(case[0], dev))
        n_points.copy_(cu(case[1], dev))
        assign.fill_(-1), eager_assign.fill_(-1)
        buf.dist.fill_(F32_FILL), eager_buf.dist.fill_(F32_FILL)

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(buf, assign)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run(buf, assign)
    assert res.plane.data_ptr() == buf.plane.data_ptr()
    for case in cases[1:] + cases[:1]:
        load(case)
        graph.replay()
        got = fit_bytes(res) + fit_bytes([assign])
        want = fit_bytes(run(eager_buf, eager_assign)) + fit_bytes([eager_assign])
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b))
        assert (got[5] == 0).all() and (got[1] > case[1] // 2).all() and int(buf.error_flag.item()) == 0
        assert ((got[6] == 3).sum(1) == got[1]).all() and (got[3][1, int(case[1][1]):] == F32_FILL).all()


def test_ground_labels_feed_euclidean_cluster(dev):
    """A flat ground lattice with two boxes standing one voxel above it: with the ground left in, 26-connectivity at 0.25 m links the
    boxes through it (one component); with ``ground_labels`` the ground rows take no part and exactly the two boxes remain."""
    g = np.mgrid[0:48, 0:48].reshape(2, -1).T / 8
    ground = np.concatenate([g, np.zeros((len(g), 1))], 1)
    box = np.mgrid[0:8, 0:8, 2:8].reshape(3, -1).T / 8
    rng = np.random.default_rng(7)
    pts = np.concatenate([ground, box + [1.0, 1.0, 0.0], box + [4.0, 3.0, 0.0]]).astype(np.float32)
    order = rng.permutation(len(pts))
    pts, is_ground = pts[order], (order < len(ground))
    d = cu(pts, dev)
    labels = plane.ground_labels(d, threshold=0.05, max_angle=15.0)
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), np.where(is_ground, -1, 0))
    with_ground, _, _ = voxel.euclidean_cluster(d, torch.zeros_like(labels), voxel_size=0.25)
    assert int(with_ground.count[0]) == 1
    comps, _, grid = voxel.euclidean_cluster(d, labels, voxel_size=0.25)
    rc = comps.row_component.cpu().numpy()
    assert int(comps.count[0]) == 2 and (rc[is_ground] == -1).all() and set(rc[~is_ground].tolist()) == {0, 1}
    assert len(set(rc[~is_ground & (pts[:, 0] < 3.0)].tolist())) == 1 and len(set(rc[~is_ground & (pts[:, 0] > 3.0)].tolist())) == 1
    grid.check()
