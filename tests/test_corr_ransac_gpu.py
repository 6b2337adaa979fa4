"""GPU: pn2_corr_ransac / pn2_corr_refit against tests/corr_ransac_ref.py at the C ABI, and registration.ransac_correspondences on top.

The bounds, stated before any run:
  * every hypothesis's twelve doubles (bit for bit: separately rounded fp64 on both sides), every hypothesis count, best_h,
    best_count, status, the error bits and the selected T EQUAL the reference's;
  * the refit's inlier count equals the reference's at the DEVICE's T;
  * the seventeen sums are the reference's terms in another order: |difference| <= count * 2^-52 * sum |term| (ICP's bound);
  * the refit's T against the header's solve (corr_ransac_ref.horn) run on the DEVICE's own sums: the bound of
    tests/test_corr_ransac_cpu.py, corr_ransac_ref.transform_tolerance (C_HORN * eps * ||N||_F / gap on the eigenvector);
  * rmse against sqrt(sums[16] / sums[0]) of the device's sums: 2^-50 relative (a division and a square root).
With half the pairs true an all-inlier triple has probability 1/8: the reference finding none among 256 has probability
0.875^256 < 1e-14, and the test asserts on the reference that it did find one."""
import numpy as np
import pytest
import torch

import corr_ransac_ref as C
from pointnet12_amd import _lib, registration

pytestmark = pytest.mark.gpu

F64_FILL, I64_FILL, I32_FILL = -123.25, -77, -55
THR = 0.02
N, M, B = 600, 650, 4
worst = {"sums": 0.0, "solve": 0.0}


def cu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


_case = {}


def case(N=N, M=M, B=B):
    """B = 4 lists of 600 pairs between 600 source rows (ld 4) and 650 target rows (ld 3), host arrays made once, read-only (other
    sizes: the same construction, B >= 4).
    Clouds 0, 1, 3: pairs 0, 2, 4, ... are true under a planted transform (the target row is float32(R p + t)), the odd ones random.
    Cloud 1's source rows lie in ONE PLANE.  Cloud 2: every pair random (all outliers).  Cloud 3 also holds a NaN source row, an inf
    target row, a target row that forty pairs share, and two pairs whose index is out of range."""
    key = (N, M, B)
    if key not in _case:
        rng = np.random.default_rng(42)
        src = np.zeros((B, N, 4), np.float32)
        src[..., :3] = rng.uniform(-2, 2, (B, N, 3))
        src[..., 3] = rng.random((B, N))
        src[1, :, 2] = np.float32(0.3) * src[1, :, 0] - np.float32(0.2) * src[1, :, 1] + np.float32(0.5)
        tgt = rng.uniform(-3, 3, (B, M, 3)).astype(np.float32)
        ps = np.tile(np.arange(N), (B, 1))
        for b in range(B):
            ps[b] = rng.permutation(N)
        pt = rng.integers(0, M, (B, N))
        truth = []
        for b in range(B):
            R, t = C.rotation(rng.normal(size=3), rng.uniform(20, 170)), rng.normal(size=3)
            truth.append(np.concatenate([R, t[:, None]], 1).reshape(12))
            if b == 2:
                continue
            rows = rng.permutation(M)[:N // 2]
            pt[b, 0::2] = rows
            tgt[b, rows] = (src[b, ps[b, 0::2], :3].astype(np.float64) @ R.T + t).astype(np.float32)
        src[3, ps[3, 10], 1] = np.nan
        tgt[3, pt[3, 21], 2] = np.inf
        pt[3, 100:140] = pt[3, 100]
        pt[3, 7], ps[3, 9] = M, -1
        for a in (src, tgt, ps, pt):
            a.setflags(write=False)
        _case[key] = dict(src=src, tgt=tgt, ps=ps.astype(np.int64), pt=pt.astype(np.int64), truth=np.stack(truth))
    return _case[key]


def sized_case(N, M=5000, B=3):
    """B = 3 lists of N pairs between N source rows (ld 4) and 5 000 target rows (ld 3), made once, read-only.  Pairs 0, 4, 8, ... are
    true under a planted transform and have a target row of their own; the others are random.  The last cloud holds a NaN source row,
    an inf target row and two pairs whose index is out of range -- none of them on a true pair."""
    key = ("sized", N, M, B)
    if key not in _case:
        rng = np.random.default_rng(N)
        true = np.arange(0, N, 4)
        assert len(true) < M
        src = np.zeros((B, N, 4), np.float32)
        src[..., :3] = rng.uniform(-2, 2, (B, N, 3))
        src[..., 3] = rng.random((B, N))
        tgt = rng.uniform(-3, 3, (B, M, 3)).astype(np.float32)
        ps = np.stack([rng.permutation(N) for _ in range(B)])
        pt = rng.integers(0, M, (B, N))
        truth = []
        for b in range(B):
            R, t = C.rotation(rng.normal(size=3), rng.uniform(20, 170)), rng.normal(size=3)
            truth.append(np.concatenate([R, t[:, None]], 1).reshape(12))
            rows = rng.permutation(M)
            pt[b, true] = rows[:len(true)]
            tgt[b, rows[:len(true)]] = (src[b, ps[b, true], :3].astype(np.float64) @ R.T + t).astype(np.float32)
            if b == B - 1:
                pt[b, 21] = rows[-1]                                 # (a row that no true pair names)
                tgt[b, rows[-1], 2] = np.inf
        src[B - 1, ps[B - 1, 10], 1] = np.nan
        pt[B - 1, 7], ps[B - 1, 9] = M, -1
        for a in (src, tgt, ps, pt):
            a.setflags(write=False)
        _case[key] = dict(src=src, tgt=tgt, ps=ps.astype(np.int64), pt=pt.astype(np.int64), truth=np.stack(truth))
    return _case[key]


class Run:
    """The case on the device with every output prefilled, and the two entry points as methods that return the code."""

    def __init__(self, dev, H, count=None, edge_ratio=0.9, seed=0, threshold=THR, c=None, fill=0xA5):
        c = case() if c is None else c
        lib = _lib.load()
        self.c, self.H, self.count_np, self.edge_ratio, self.seed, self.threshold = c, H, count, edge_ratio, seed, threshold
        (self.B, self.N), self.M = c["ps"].shape, c["tgt"].shape[1]
        B, N = self.B, self.N
        self.src, self.tgt, self.ps, self.pt = (cu(c[k], dev) for k in ("src", "tgt", "ps", "pt"))
        self.count = None if count is None else cu(np.int64(count), dev)
        self.work = torch.full((lib.pn2_corr_workspace_bytes(B, N, H),), fill, device=dev, dtype=torch.uint8)           # (it may hold anything)
        f = lambda shape, v, dt: torch.full(shape, v, device=dev, dtype=dt)
        self.out = dict(T=f((B, 12), F64_FILL, torch.float64), hyp=f((B, H, 12), F64_FILL, torch.float64), hyp_count=f((B, H), I32_FILL, torch.int32),
                        best_h=f((B,), I32_FILL, torch.int32), best_count=f((B,), I64_FILL, torch.int64), status=f((B,), I32_FILL, torch.int32),
                        err=f((1,), 0, torch.int32), inliers=f((B,), I64_FILL, torch.int64), rmse=f((B,), F64_FILL, torch.float64),
                        sums=f((B, C.SUMS), F64_FILL, torch.float64))

    def clouds(self):
        p = _lib.ptr
        return (p(self.src), 4, p(self.tgt), 3, self.B, self.N, self.M, p(self.ps), p(self.pt), p(self.count))

    def ransac(self):
        p, o = _lib.ptr, self.out
        return _lib.load().pn2_corr_ransac(*self.clouds(), self.H, self.seed, self.edge_ratio, self.threshold, p(o["T"]), p(o["hyp"]), p(o["hyp_count"]),
                                           p(o["best_h"]), p(o["best_count"]), p(o["status"]), p(o["err"]), p(self.work), _lib.stream())

    def refit(self, flags=0):
        p, o = _lib.ptr, self.out
        return _lib.load().pn2_corr_refit(*self.clouds(), self.threshold, flags, p(o["T"]), p(o["inliers"]), p(o["rmse"]), p(o["sums"]), p(o["status"]),
                                          p(self.work), _lib.stream())

    def host(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def counts(self):
        return np.full(self.B, self.N, np.int64) if self.count_np is None else np.clip(np.int64(self.count_np), 0, self.N)

    def reference(self):
        c = self.c
        return C.ransac(c["src"], c["tgt"], c["ps"], c["pt"], self.threshold, self.H, self.seed, self.edge_ratio, self.count_np)


def check_ransac(got, ref):
    nan = np.isnan(ref["hyp"])                                       # (an invalid hypothesis: twelve NaNs on both sides)
    assert np.array_equal(np.isnan(got["hyp"]), nan) and np.array_equal(bits(got["hyp"][~nan]), bits(ref["hyp"][~nan]))
    assert np.array_equal(got["hyp_count"], ref["hyp_count"])
    assert np.array_equal(got["best_h"], ref["best_h"]) and np.array_equal(got["best_count"], ref["best_count"])
    assert np.array_equal(got["status"], ref["status"]) and int(got["err"][0]) == ref["err"]
    assert np.array_equal(bits(got["T"]), bits(ref["T"]))


@pytest.mark.parametrize("H", [1, 100, 256, 1000])
@pytest.mark.parametrize("edge_ratio", [0.0, 0.9])
def test_ransac_equals_the_reference(dev, H, edge_ratio):
    """Every row; a device-side count below 600; the counts 0, 2 and 3.  Two runs write the same bytes."""
    for count in (None, [600, 431, 599, 9000], [0, 2, 3, 600]):
        r = Run(dev, H, count, edge_ratio)
        assert r.ransac() == 0
        got = r.host()
        ref = r.reference()
        check_ransac(got, ref)
        again = Run(dev, H, count, edge_ratio)
        assert again.ransac() == 0
        second = again.host()
        assert all(np.array_equal(bits(got[k]), bits(second[k])) for k in ("T", "hyp", "hyp_count", "best_h", "best_count", "status", "err"))
        if count is not None and count[0] == 0:
            assert (ref["status"][:2] == C.NONE).all() and (ref["hyp_count"][:2] == -1).all() and ref["best_h"][0] == -1 and ref["err"] & C.ERR_NONE
            assert (got["T"][0] == C.IDENTITY).all()
        if count is None:
            assert ref["err"] & C.ERR_PAIR and ref["err"] & C.ERR_NONFINITE
            if H >= 256:
                assert (ref["best_count"][[0, 1, 3]] >= 250).all() and (ref["status"][[0, 1, 3]] == 0).all()        # an all-inlier triple was found
                assert ref["best_count"][2] < 20                     # the cloud of outliers: whatever wins, wins by chance
            if H == 256:
                valid = (ref["hyp_count"] >= 0).sum(1)
                assert (valid[[0, 1, 3]] > 0).all() and (edge_ratio == 0.0 or (valid < 128).all())          # the edge test does drop hypotheses


def check_refit(r, got, T_in, status_in):
    c = r.c
    ns = r.counts()
    for b in range(r.B):
        if status_in[b] & C.NONE:
            assert (got["sums"][b] == F64_FILL).all() and got["rmse"][b] == F64_FILL and got["inliers"][b] == I64_FILL
            assert np.array_equal(bits(got["T"][b]), bits(T_in[b]))
            continue
        ref = C.refit(c["src"][b], c["tgt"][b], c["ps"][b], c["pt"][b], int(ns[b]), T_in[b], r.threshold)
        S = got["sums"][b]
        assert got["inliers"][b] == ref["count"] and S[0] == ref["count"]
        diff, bound = np.abs(S - ref["sums"]), ref["count"] * 2.0 ** -52 * ref["abs_sums"]
        worst["sums"] = max(worst["sums"], float((diff / np.maximum(bound, 1e-300)).max()))
        assert (diff <= bound).all()
        assert abs(got["rmse"][b] - C.rmse_of(S)) <= 2.0 ** -50 * C.rmse_of(S)
        want, degenerate = C.horn(S)
        assert bool(got["status"][b] & C.DEGENERATE) == degenerate or bool(status_in[b] & C.DEGENERATE)
        if degenerate:
            assert np.array_equal(bits(got["T"][b]), bits(T_in[b]))
            continue
        tol = C.transform_tolerance(S)
        err = np.abs(got["T"][b] - want)
        worst["solve"] = max(worst["solve"], float((err / tol).max()))
        assert (err <= tol).all()


def test_refit_rounds(dev):
    """Two refit rounds and a closing evaluation after a RANSAC with 256 hypotheses: generic inliers (cloud 0), inliers in one plane
    (cloud 1), a cloud with PN2_CORR_NONE (cloud 2: threshold-sized luck aside, its count may reach 3, then it is refitted like the
    others) and the cloud with broken pairs (cloud 3)."""
    c = case()
    for count in (None, [600, 431, 2, 600]):
        r = Run(dev, 256, count)
        assert r.ransac() == 0
        got = r.host()
        for _ in range(2):
            T_in, status_in = got["T"].copy(), got["status"].copy()
            assert r.refit() == 0
            got = r.host()
            check_refit(r, got, T_in, status_in)
        for b in (0, 1, 3):                                          # the refitted transform is the planted one
            assert np.abs(got["T"][b] - c["truth"][b]).max() <= 1e-5 and got["inliers"][b] >= (200 if b == 1 and count else 270)
        T_in, sums_in = got["T"].copy(), got["sums"].copy()
        assert r.refit(_lib.CORR_EVAL_ONLY) == 0
        last = r.host()
        assert np.array_equal(bits(last["T"]), bits(T_in)) and np.array_equal(last["status"], got["status"])
        for b in (0, 1, 3):
            assert last["sums"][b, 0] == last["inliers"][b] >= 200 and last["rmse"][b] <= 1e-5
        assert r.refit(_lib.CORR_EVAL_ONLY) == 0
        assert all(np.array_equal(bits(v), bits(last[k])) for k, v in r.host().items())          # two runs, the same bytes
        if count is not None:
            assert got["status"][2] & C.NONE
    print("worst sums %.3f of the bound, worst solve %.3f of the tolerance" % (worst["sums"], worst["solve"]))


# Past one tile: 2 refit tiles (1 025 pairs), 9 and 17 (the finish kernel's thread (k, c) adds word k of tiles c, c + 8, c + 16, ...), with
# B = 3 so that ``partial``'s pitch is exercised with more than one tile.  Counts: cloud 1 ends exactly on a tile boundary with whole
# tiles of the launch beyond it, cloud 2 ends inside a tile.  The sampler's seeds are chosen on the reference alone so that an
# all-inlier triple is among the 257 hypotheses of every cloud (a quarter of the pairs is true: one triple in 64).
SEAM_CASES = {1025: ((1025, 1024, 600), 0), 8193: ((8193, 8192, 5000), 0), 16385: ((16385, 8192, 9000), 0)}        # N: counts, seed
SEAM_H = 257


def true_pairs(counts):
    return (np.int64(counts) + 3) // 4                               # pairs 0, 4, 8, ... below each count


def run_seam(dev, N):
    """RANSAC, two refit rounds and a closing evaluation of ``sized_case(N)`` on a workspace of 0xFF bytes, every stage checked
    -> the outputs after each stage."""
    counts, seed = SEAM_CASES[N]
    r = Run(dev, SEAM_H, list(counts), seed=seed, c=sized_case(N), fill=0xFF)
    assert r.ransac() == 0
    got = r.host()
    ref = r.reference()
    assert np.array_equal(ref["best_count"], true_pairs(counts)) and (ref["status"] == 0).all()       # (the input's condition)
    assert ref["err"] == C.ERR_PAIR | C.ERR_NONFINITE
    check_ransac(got, ref)
    stages = [got]
    for _ in range(2):
        T_in, status_in = got["T"].copy(), got["status"].copy()
        assert r.refit() == 0
        got = r.host()
        check_refit(r, got, T_in, status_in)
        stages.append(got)
    assert (got["status"] == 0).all() and np.array_equal(got["inliers"], true_pairs(counts))
    assert np.abs(got["T"] - r.c["truth"]).max() <= 1e-5            # the refitted transform is the planted one
    T_in = got["T"].copy()
    assert r.refit(_lib.CORR_EVAL_ONLY) == 0
    last = r.host()
    assert np.array_equal(bits(last["T"]), bits(T_in)) and np.array_equal(last["status"], got["status"])
    for b in range(r.B):
        ev = C.refit(r.c["src"][b], r.c["tgt"][b], r.c["ps"][b], r.c["pt"][b], int(counts[b]), T_in[b], r.threshold)
        assert last["inliers"][b] == last["sums"][b, 0] == ev["count"]
        assert (np.abs(last["sums"][b] - ev["sums"]) <= ev["count"] * 2.0 ** -52 * ev["abs_sums"]).all()
        assert abs(last["rmse"][b] - C.rmse_of(last["sums"][b])) <= 2.0 ** -50 * C.rmse_of(last["sums"][b])
    return stages + [last]


@pytest.mark.parametrize("N", sorted(SEAM_CASES))
def test_ransac_and_refit_past_one_tile(dev, N):
    first, second = run_seam(dev, N), run_seam(dev, N)
    for a, b in zip(first, second):
        assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)          # two runs, the same bytes
    print("worst sums %.3f of the bound, worst solve %.3f of the tolerance" % (worst["sums"], worst["solve"]))


def test_refit_degenerate_and_arguments(dev):
    r = Run(dev, 64, [600, 600, 600, 600], threshold=0.0)           # threshold 0: a float32 target row is never exactly R p + t
    assert r.ransac() == 0
    got = r.host()
    check_ransac(got, r.reference())
    r.out["status"].zero_()                                          # refit whatever T holds: no pair within 0 -> fewer than 3 inliers
    T_in = r.host()["T"].copy()
    assert r.refit() == 0
    got = r.host()
    assert (got["status"] == C.DEGENERATE).all() and np.array_equal(bits(got["T"]), bits(T_in)) and (got["inliers"] < 3).all()
    lib = _lib.load()
    assert lib.pn2_corr_workspace_bytes(0, 10, 10) == -1 and lib.pn2_corr_workspace_bytes(1, 10, 0) == -1 and lib.pn2_corr_workspace_bytes(1, 10, 65537) == -1
    bad = Run(dev, 16)
    bad.edge_ratio = 1.5
    assert bad.ransac() == -1
    bad.edge_ratio, bad.threshold = 0.9, float("nan")
    assert bad.ransac() == -1 and bad.refit() == -1 and bad.refit(2) == -1
    torch.cuda.synchronize()
    assert (bad.out["T"] == F64_FILL).all() and (bad.out["status"] == I32_FILL).all()


def test_ransac_correspondences_python_layer(dev):
    """registration.ransac_correspondences on cloud 0 ([N,ld] inputs) and on the batch with buffers: the planted transform comes
    back, the closing evaluation counts the true pairs, check() names the broken pairs of cloud 3."""
    c = case()
    src, tgt, ps, pt = (cu(c[k], dev) for k in ("src", "tgt", "ps", "pt"))
    res = registration.ransac_correspondences(src[0], tgt[0], (ps[0], pt[0], None), THR, iterations=256)
    assert res.transform.shape == (4, 4) and int(res.status) == 0 and int(res.count) >= 300 and float(res.rmse) <= 1e-5
    assert np.abs(res.transform.cpu().numpy()[:3].reshape(12) - c["truth"][0]).max() <= 1e-5
    moved = registration.transform_points(src[0], res.transform).cpu().numpy().astype(np.float64)
    assert np.abs(moved - C.apply(c["truth"][0], c["src"][0, :, :3].astype(np.float64))).max() <= 1e-4
    buf = registration.corr_buffers(N, B=B, iterations=256, device=dev)
    count = cu(np.int64([600, 600, 2, 600]), dev)
    res = registration.ransac_correspondences(src, tgt, (ps, pt, count), THR, iterations=256, buffers=buf)
    assert res.transform is buf.transform and res.status.tolist() == [0, 0, C.NONE, 0] and res.count[2] == 0
    assert torch.equal(res.transform[2], torch.eye(4, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        buf.check()                                                  # cloud 3's pairs
    with pytest.raises(ValueError):
        registration.ransac_correspondences(src, tgt, (ps, pt, count), THR, iterations=128, buffers=buf)
