"""CPU: the numpy restatement of the device scan filter's rule (tests/scan_filter_ref.py) against what the reference's own
``Semantic_KITTI_Utils.get`` returned (tests/golden/g9_kitti.npz) and against ``kitti.in_view``; the argument checks of
``pn2_scan_filter``, which launch nothing."""
import ctypes

import numpy as np
import pytest

import scan_filter_ref as R
from conftest import golden
from pointnet12_amd import _lib, kitti

G9_MAX_UNDECIDED = 2          # of 7 513 points, at w = 4 (counted when the fixture was first put through the restatement: 2)


def g9():
    g = golden("g9_kitti.npz")
    return g, R.make_lut({int(k): int(v) for k, v in zip(g["map_keys"], g["map_values"])})


@pytest.mark.parametrize("subset", ["all", "inview"])
def test_restatement_against_the_recorded_scan(subset):
    g, lut = g9()
    fov = R.thresholds() if subset == "inview" else None
    box = R.DEFAULT_BOX if subset == "inview" else None
    got = R.scan_filter(g["bin"], g["label"], lut, fov, box, w=4)
    rec = R.recorded_mask(g["bin"], g["label"], g[subset + "/points"], g[subset + "/labels"], lut)
    und = got["undecided"]
    print("g9 %s: %d kept, %d undecided at w = 4, %d differ, %d differ outside the band"
          % (subset, got["mask"].sum(), und.sum(), (got["mask"] != rec).sum(), ((got["mask"] != rec) & ~und).sum()))
    assert not got["unmapped"]
    assert int(und.sum()) <= G9_MAX_UNDECIDED
    assert not ((got["mask"] != rec) & ~und).any()
    if not (got["mask"] != rec).any():                              # then the compacted rows are the recorded ones, bit for bit
        assert np.array_equal(got["points"].view(np.uint32), g[subset + "/points"].view(np.uint32))
        assert np.array_equal(got["labels"], g[subset + "/labels"])
    assert (np.diff(got["index"]) > 0).all() and np.array_equal(got["index"], np.flatnonzero(got["mask"]))


def test_restatement_against_in_view_on_random_points():
    rng = np.random.default_rng(20)
    pts = (rng.normal(size=(2_000_000, 4)) * np.array([40.0, 40.0, 6.0, 1.0])).astype(np.float32)
    ref = kitti.in_view(pts)
    got = R.scan_filter(pts, None, None, R.thresholds(), R.DEFAULT_BOX, w=4)
    differ = got["mask"] != ref
    print("2 M random points: %d differ, %d undecided at w = 4, %d differ outside the band"
          % (differ.sum(), got["undecided"].sum(), (differ & ~got["undecided"]).sum()))
    assert not (differ & ~got["undecided"]).any()
    assert got["undecided"].mean() < 1e-4                            # the band is a sliver: the comparison above is not vacuous
    assert 0.05 < ref.mean() < 0.5


def test_special_values_in_the_restatement():
    inf, nan = np.inf, np.nan
    pts = np.array([[0, 0, 0, 0], [-0.0, 0.0, 0, 0], [0.0, -0.0, 0, 0], [nan, 0, 0, 0], [1, inf, 0, 0], [1, 0, -inf, 0], [5, 0, 0, 0]], np.float32)
    got = R.scan_filter(pts, None, None, R.thresholds(), R.DEFAULT_BOX)
    assert got["mask"].tolist() == [True, False, True, False, False, False, True]      # az(-0, +0) = pi: dropped


def test_sweeps_keep_their_band_small():
    """The border sweeps of the GPU test: at w = 1 the restatement's own band holds under 1 % of each sweep, and each sweep
    does cross its threshold."""
    t = R.thresholds()
    for name, (pts, i) in R.sweeps().items():
        got = R.scan_filter(pts, None, None, t, R.DEFAULT_BOX, w=1)
        frac = got["undecided"].mean()
        print("sweep %s: %d kept of %d, %d in the w = 1 band" % (name, got["mask"].sum(), len(pts), got["undecided"].sum()))
        assert 0 < frac < 0.01, name
        assert 0.4 < got["mask"].mean() < 0.6, name
        assert (np.diff(pts[:, 2 if i >= 2 else 1].astype(np.float64)) >= 0).all()


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    ws = lib.pn2_scan_filter_workspace_bytes
    assert ws(0, 100) == -1 and ws(1, -1) == -1 and ws(1, 2 ** 31) == -1 and ws(70000, 100) == -1
    T = _lib.SCAN_TILE
    assert ws(1, 0) == ws(1, 1) == ws(1, T) == T + 2 * 16
    assert ws(3, 5 * T + 1) == 3 * 6 * T + 2 * ((3 * 6 * 4 + 15) // 16 * 16)
    assert ws(1, 2 ** 31 - 1) > 2 ** 31
    a = ctypes.c_void_p(4096)              # a plausible (never dereferenced) aligned address: every call below returns before a launch
    fov = (ctypes.c_float * 4)(-1, 1, -1, 1)
    box = (ctypes.c_float * 8)(*R.DEFAULT_BOX)
    ok = dict(raw=a, label=a, begin=a, count=a, B=1, max_rows=100, lut=a, lut_len=260, fov=fov, box=box, out_begin=a, pts=a, lab=a,
              idx=a, cnt=a, err=a, ws=a)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.pn2_scan_filter(v["raw"], v["label"], v["begin"], v["count"], v["B"], v["max_rows"], v["lut"], v["lut_len"], v["fov"],
                                   v["box"], v["out_begin"], v["pts"], v["lab"], v["idx"], v["cnt"], v["err"], v["ws"], None)
    for bad in (dict(raw=None), dict(begin=None), dict(count=None), dict(out_begin=None), dict(pts=None), dict(cnt=None), dict(ws=None),
                dict(B=0), dict(B=-3), dict(max_rows=-1), dict(max_rows=2 ** 31), dict(lut_len=0), dict(lut=None),
                dict(raw=ctypes.c_void_p(4100)), dict(pts=ctypes.c_void_p(4104))):
        assert call(**bad) == -1, bad


def test_scan_filter_refuses_the_cpu():
    with pytest.raises(_lib.Pn2Error):
        kitti.ScanFilter({0: 0, 1: 1}, device="cpu")
    with pytest.raises(AssertionError):
        kitti.ScanFilter({0: 0, 1: 1}, subset="front", device="cpu")
