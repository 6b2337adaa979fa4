"""CPU: the voxel-grid rule (include/pn2.h, ``pn2_voxel_grid``) as tests/voxel_ref.py states it, held to a brute-force restatement,
to planted border values and to the recorded scan; the entry point's argument checks (no launch, no GPU) and the "no scratch"
check of csrc/voxel.hip."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import voxel_ref as R
from conftest import ROOT, golden
from pointnet12_amd import _lib


@pytest.mark.parametrize("seed,M,voxel,origin", [(0, 300, 0.5, 0.0), (1, 257, (0.3, 0.7, 1.1), (0.25, -3.0, 1e-3)), (2, 1, 1.0, 0.0),
                                                 (3, 120, 4.0, 0.0)])
def test_restatement_against_brute_force(seed, M, voxel, origin):
    rng = np.random.default_rng(seed)
    pts = rng.normal(scale=1.5, size=(M, 4)).astype(np.float32)
    if M > 10:
        pts[5, 1], pts[7, 0], pts[9, 2] = np.nan, np.inf, 1e30        # invalid rows, one of them low enough to shift ranks
        pts[20:30] = pts[3]                                           # exact duplicates
    labels = rng.integers(0, 19, M).astype(np.int32)
    ref = R.voxel_grid(pts, origin, voxel, labels)
    index, inverse, n_points = R.brute_force(pts, origin, voxel)
    assert np.array_equal(ref["index"], index) and np.array_equal(ref["inverse"], inverse) and np.array_equal(ref["n_points"], n_points)
    assert ref["count"] == len(index) and (np.diff(ref["index"]) > 0).all()
    assert np.array_equal(ref["points"].view(np.uint32), pts[index].view(np.uint32)) and np.array_equal(ref["labels"], labels[index])
    assert ref["n_points"].sum() == ref["valid"].sum() and (ref["inverse"] >= 0).sum() == ref["valid"].sum()
    key, valid = R.keys(pts, origin, voxel)
    expect = np.flatnonzero(valid)[np.sort(np.unique(key[valid], return_index=True)[1])]
    assert np.array_equal(ref["index"], expect)


def cell_x(value, voxel, origin=0.0):
    q, valid = R.cells(np.array([[value, 0.0, 0.0]], np.float32), origin, voxel)
    assert valid[0]
    return q[0, 0]


def test_planted_values():
    assert cell_x(np.float32(0.1), 0.1) == 1.0                        # float32(0.1) lies just ABOVE the fp64 0.1
    assert cell_x(np.float32(0.3), 0.1) == 3.0
    assert cell_x(-0.05, 0.1) == -1.0
    q = cell_x(-0.0, 0.1)
    assert q == 0.0 and np.signbit(q)                                 # floor(-0.0) = -0.0: cell 0
    key, valid = R.keys(np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0]], np.float32), 0.0, 0.1)
    assert valid.all() and key[0] == key[1] == (R.LIMIT << 42) | (R.LIMIT << 21) | R.LIMIT
    for k in range(-40, 41):                                          # exact multiples: the cell is the multiple, either sign
        assert cell_x(k * 0.125, 0.125) == float(k)
    # the valid range, compared in fp64: cells -2^20 and 2^20 - 1 are inside, -2^20 - 1 and 2^20 are not; NaN / inf / 1e30 neither
    pts = np.array([[-1048576.0, 0, 0], [1048575.0, 0, 0], [-1048577.0, 0, 0], [1048576.0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0],
                    [0, 0, -np.inf], [1e30, 0, 0]], np.float32)
    key, valid = R.keys(pts, 0.0, 1.0)
    assert valid.tolist() == [True, True, False, False, False, False, False, False]
    assert key[0] >> 42 == 0 and key[1] >> 42 == (1 << 21) - 1 and key[1] < (1 << 63)


def test_recorded_scan_counts():
    """The recorded scan (7 513 rows): voxel counts under this rule, computed with numpy."""
    raw = np.ascontiguousarray(golden("g9_kitti.npz")["bin"])
    assert raw.shape == (7513, 4)
    ref = R.voxel_grid(raw, 0.0, 0.1)
    assert ref["count"] == 4800 and ref["n_points"].max() <= 10 and ref["valid"].all() and ref["n_points"].sum() == 7513
    for size, count in ((0.05, 5133), (0.2, 4116), (0.5, 3105)):
        assert R.voxel_grid(raw, 0.0, size)["count"] == count


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    d3 = lambda *v: (ctypes.c_double * 3)(*v)
    org, vox = d3(0, 0, 0), d3(0.1, 0.1, 0.1)
    a = 4096                                                          # a non-null, aligned stand-in: a refused call touches nothing
    vp = lambda x: ctypes.c_void_p(x)

    def call(pts=a, ld=4, B=1, max_rows=16, origin=org, voxel=vox, out_count=a, workspace=a, begin=a):
        return lib.pn2_voxel_grid(vp(pts), ld, None, vp(begin), vp(a), B, max_rows, origin, voxel, vp(a), None, None, None,
                                  vp(out_count), None, None, None, vp(workspace), None)
    EINVAL = -1
    assert call(pts=None) == EINVAL and call(out_count=None) == EINVAL and call(workspace=None) == EINVAL
    assert call(begin=None) == EINVAL and call(origin=None) == EINVAL and call(voxel=None) == EINVAL
    assert call(B=0) == EINVAL and call(B=-3) == EINVAL and call(B=65536) == EINVAL
    assert call(ld=2) == EINVAL and call(ld=17) == EINVAL
    assert call(max_rows=-1) == EINVAL and call(max_rows=_lib.VOXEL_MAX_ROWS + 1) == EINVAL
    assert call(voxel=d3(0.1, 0.0, 0.1)) == EINVAL and call(voxel=d3(0.1, 0.1, -1.0)) == EINVAL
    assert call(voxel=d3(float("nan"), 0.1, 0.1)) == EINVAL and call(voxel=d3(0.1, float("inf"), 0.1)) == EINVAL
    assert call(origin=d3(0, float("nan"), 0)) == EINVAL and call(origin=d3(float("-inf"), 0, 0)) == EINVAL
    assert call(pts=a + 2) == EINVAL and call(workspace=a + 8) == EINVAL                    # alignment: 4 bytes, 16 bytes
    wb = lib.pn2_voxel_grid_workspace_bytes
    assert wb(0, 16) == EINVAL and wb(1, -1) == EINVAL and wb(65536, 16) == EINVAL and wb(1, _lib.VOXEL_MAX_ROWS + 1) == EINVAL
    assert _lib.VOXEL_MAX_ROWS >= 1 << 22 and wb(1, 1 << 22) > 0 and wb(1, 0) > 0
    sizes = [wb(1, m) for m in (0, 1, 63, 1024, 1025, 4096, 120000, 131071, 1 << 22)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)              # monotone in max_rows
    by_b = [wb(B, 5000) for B in (1, 2, 3, 16, 65535)]
    assert all(s > 0 and s % 16 == 0 for s in by_b) and by_b == sorted(set(by_b))            # ... and strictly in B
    for m in (1, 1000, 120000):                                       # a table of at least 2 * max_rows 16-byte slots, 5 bytes a row
        assert wb(1, m) >= 2 * m * 16 + 5 * m


# pn2_scan_filter_workspace_bytes, pn2_voxel_grid_workspace_bytes and pn2_segment_reduce_workspace_bytes as the library returned them
# BEFORE the three files shared compact.h / slot_table.h (recorded from that build, not computed): callers size allocations by them.
WS_MAX_ROWS = (0, 1, 1023, 1024, 1025, 120000, 1 << 29)
WS_SCAN = {
    1: [1056, 1056, 1056, 1056, 2080, 121792, 541065216],
    3: [3104, 3104, 3104, 3104, 6208, 365344, 1623195648],
    16: [16512, 16512, 16512, 16512, 33024, 1948416, 8657043456],
}
WS_VOXEL = {
    1: [6176, 6176, 37920, 37920, 75808, 4799424, 19868418048],
    3: [18464, 18464, 113696, 113696, 227392, 14398240, 59605254144],
    16: [98432, 98432, 606336, 606336, 1212672, 76790528, 317894688768],
}
WS_SEGMENT = {                                                        # (B, C)
    (1, 1): [1024, 1040, 40960, 40960, 73744, 5154304, 21474836480],
    (1, 4): [1024, 1040, 53200, 53248, 73744, 6240000, 27917287424],
    (1, 16): [1024, 1040, 200512, 200704, 200912, 23520000, 105226698752],
    (3, 1): [3072, 3104, 122864, 122880, 221216, 15462912, 64424509440],
    (3, 4): [3072, 3104, 159600, 159744, 221216, 18720000, 83751862272],
    (3, 16): [3072, 3104, 601536, 602112, 602704, 70560000, 315680096256],
    (16, 1): [16384, 16512, 655232, 655360, 1179776, 82468864, 343597383680],
    (16, 4): [16384, 16512, 851136, 851968, 1179776, 99840000, 446676598784],
    (16, 16): [16384, 16512, 3208128, 3211264, 3214400, 376320000, 1683627180032],
}


def test_workspace_sizes_are_the_recorded_ones():
    lib = _lib.load()
    scan, voxel, segment = lib.pn2_scan_filter_workspace_bytes, lib.pn2_voxel_grid_workspace_bytes, lib.pn2_segment_reduce_workspace_bytes
    for B, want in WS_SCAN.items():
        assert [scan(B, m) for m in WS_MAX_ROWS] == want
    for B, want in WS_VOXEL.items():
        assert [voxel(B, m) for m in WS_MAX_ROWS] == want
    for (B, C), want in WS_SEGMENT.items():
        assert [segment(B, m, C) for m in WS_MAX_ROWS] == want
    EINVAL = -1
    assert scan(0, 16) == EINVAL and scan(65536, 16) == EINVAL and scan(1, 1 << 31) == EINVAL
    assert scan(1, (1 << 31) - 1) == 2164260864 and scan(1, (1 << 29) + 1) == 541066272      # (the filter's own limit is 2^31 - 1)
    assert voxel(0, 16) == EINVAL and voxel(65536, 16) == EINVAL and voxel(1, (1 << 29) + 1) == EINVAL
    assert segment(0, 16, 4) == EINVAL and segment(65536, 16, 4) == EINVAL and segment(1, (1 << 29) + 1, 4) == EINVAL
    assert segment(1, 16, 0) == EINVAL and segment(1, 16, 17) == EINVAL


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_voxel_kernels_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "voxel.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
