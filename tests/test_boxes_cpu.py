"""CPU: the segment-box rule (include/pn2.h, "segment boxes") as tests/box_ref.py states it -- the reference itself, held to
constructions whose answer is known -- plus the plain-torch helpers of pointnet12_amd/boxes.py and what needs no GPU of the binding.
tests/test_boxes_gpu.py holds csrc/boxes.hip to box_ref, bit for bit."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_ref as R
from conftest import ROOT
from pointnet12_amd import _lib, boxes

STEP = 90.0 / 64                                                     # one table step of A = 64, in degrees: 1.40625


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rotated(P, a, A=64, shift=(12.0, -7.0)):
    th = a * (math.pi / 2) / A
    Rm = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    return (P @ Rm.T + np.asarray(shift)).astype(np.float32)


def one(points_xy, table, d0=0.05):
    pts = np.concatenate([points_xy, np.zeros((len(points_xy), 1), np.float32)], 1)
    return R.segment_boxes(pts, np.zeros(len(pts), np.int32), 1, table, d0)


@pytest.mark.parametrize("shape", ["lattice", "L"])
def test_lattices_at_table_angles(shape):
    """A 21 x 10 lattice of 0.2 m pitch (and its L: the bottom edge plus the right edge) rotated in fp64 by every angle of the table:
    the sweep names that angle, 64 times out of 64."""
    T = R.angle_table(64)
    ii, jj = (g.ravel() for g in np.meshgrid(np.arange(21), np.arange(10), indexing="ij"))
    P = np.stack([ii * 0.2, jj * 0.2], 1)
    if shape == "L":
        P = P[(jj == 0) | (ii == 20)]
    for a in range(64):
        got = one(rotated(P, a), T)
        assert got["angle"][0] == a and got["yaw"][0] == T[a, 2]
        assert abs(got["size"][0, 0] - 4.0) < 1e-4 and abs(got["size"][0, 1] - 1.8) < 1e-4


def l_shape_errors(d0):
    rng = np.random.default_rng(0)
    T = R.angle_table(64)
    err = []
    for _ in range(150):
        yaw, n = rng.uniform(0, math.pi / 2), int(rng.integers(30, 121))
        got = R.segment_boxes(R.car_l_shape(rng, n, yaw), np.zeros(n, np.int32), 1, T, d0)
        err.append(R.yaw_error_deg(got["yaw"][0], yaw))
    return np.array(err)


def test_l_shape_closeness_against_area():
    """150 seeded L-shaped clusters of a 4.2 x 1.8 m car at 12 m, 30 .. 120 points, sigma = 2 cm.  Closeness: the median yaw error
    within one table step, at most 5 % of the scenes beyond two (measured at this seed: median 0.37, 95th percentile 0.81, max 1.18
    degrees).  The minimum-area rectangle on the SAME scenes: a median above 10 degrees (measured 22.2) -- the hull of an L is a right
    triangle, and its rectangle flush with a leg ties with the one flush with the hypotenuse.  Why the default is what it is."""
    close, area = l_shape_errors(0.05), l_shape_errors(0.0)
    assert np.median(close) <= STEP and (close > 2 * STEP).mean() <= 0.05
    assert np.median(area) > 10.0


def test_row_order_changes_no_bit_and_zero_signs_follow_the_key_order():
    rng = np.random.default_rng(3)
    T = R.angle_table(64)
    pts = np.concatenate([R.car_l_shape(rng, 80, 0.3), R.car_l_shape(rng, 45, 1.1, centre=(-6.0, 9.0))], 0)
    seg = np.concatenate([np.zeros(80, np.int32), np.ones(45, np.int32)])
    ref = R.segment_boxes(pts, seg, 2, T)
    for _ in range(3):
        perm = rng.permutation(len(pts))
        got = R.segment_boxes(pts[perm], seg[perm], 2, T)
        for name in ("center", "size", "yaw", "lo", "hi"):
            assert np.array_equal(u32(got[name]), u32(ref[name])), name
        for name in ("angle", "n", "score"):
            assert np.array_equal(got[name], ref[name]), name
    # -0.0 < +0.0 in the key order: the minimum of {-0.0, +0.0} is -0.0, the maximum +0.0, whatever the order of the rows
    assert R.key(np.float32(-0.0)) < R.key(np.float32(0.0)) and R.key(np.float32(-1e-45)) < R.key(np.float32(-0.0))
    z = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]], np.float32)
    for rows in (z, z[::-1]):
        got = R.segment_boxes(rows, [0, 0], 1, R.angle_table(1))
        assert (u32(got["lo"]) == 0x80000000).all() and (u32(got["hi"]) == 0).all()
    f = rng.normal(size=1000).astype(np.float32)
    assert np.array_equal(R.unkey(R.key(f)).view(np.uint32), f.view(np.uint32)) and (np.argsort(R.key(f), kind="stable") == np.argsort(f, kind="stable")).all()


def disc():
    g = np.arange(-3, 4)
    X, Y = np.meshgrid(g, g)
    m = X ** 2 + Y ** 2 <= 9
    return X[m].astype(np.float32), Y[m].astype(np.float32)


def test_ties_go_to_the_smaller_area_and_then_the_lowest_angle():
    """The lattice points of the disc x^2 + y^2 <= 9 are symmetric under (x, y) -> (y, x), and the table under a -> A - a bit for bit
    (c_a == s_(A - a)): angles 19 and 45 tie in score AND in area (28.851322), and 19 is returned."""
    T = R.angle_table(64)
    assert all(T[a, 0].tobytes() == T[64 - a, 1].tobytes() for a in range(1, 64))
    x, y = disc()
    for d0 in (0.05, 0.0):
        a, score, _, _, _, _, area, scores = R.fit(x, y, T, d0)
        assert a == 19 and scores[19] == scores[45] == scores.max() and u32(area[19]) == u32(area[45]) == u32(np.float32(28.851322))
        assert set(np.flatnonzero((scores == scores.max()) & (area == area[19]))) == {19, 45}
    # the area only breaks score ties: a lower score with a smaller area loses
    assert R.fit(x, y, T, 0.05)[1] > 0 and R.fit(x, y, T, 0.0)[1] == 0
    # identical points: size 0, every angle ties, angle 0
    same = np.tile(np.array([[3.25, -1.5, 0.75]], np.float32), (9, 1))
    got = R.segment_boxes(same, np.zeros(9, np.int32), 1, T)
    assert got["angle"][0] == 0 and not got["size"].any() and np.array_equal(got["center"][0], same[0]) and got["n"][0] == 9


def test_rows_that_take_no_part():
    rng = np.random.default_rng(5)
    T = R.angle_table(64)
    pts = R.car_l_shape(rng, 60, 0.7)
    seg = np.zeros(60, np.int32)
    ref = R.segment_boxes(pts, seg, 2, T)
    assert ref["err"] == 0 and ref["angle"].tolist()[1] == -1 and ref["n"].tolist() == [60, 0]
    for col, value in ((0, np.nan), (1, np.inf), (2, -np.inf), (0, 2.0 ** 61), (1, -2.0 ** 61), (2, np.nan)):
        bad = np.concatenate([pts, pts[:1]], 0)
        bad[-1, col] = value
        got = R.segment_boxes(bad, np.zeros(61, np.int32), 2, T)
        assert got["err"] == R.ERR_NONFINITE and got["n"][0] == 60
        for name in ("center", "size", "yaw", "lo", "hi", "angle", "score"):
            assert np.array_equal(got[name], ref[name]), (name, col, value)
    edge = np.concatenate([pts, [[2.0 ** 60, -2.0 ** 60, 3e38]]], 0).astype(np.float32)      # the largest magnitudes that take part
    got = R.segment_boxes(edge, np.zeros(61, np.int32), 1, T)
    assert got["err"] == 0 and got["n"][0] == 61 and np.isfinite(got["size"][0, :2]).all()
    # a negative segment sets nothing, one at or beyond the count the RANGE bit; neither is looked at
    bad = pts.copy()
    bad[3] = np.nan
    s = seg.copy()
    s[3] = -1
    assert R.segment_boxes(bad, s, 1, T)["err"] == 0
    s[3] = 1
    assert R.segment_boxes(bad, s, 1, T)["err"] == R.ERR_RANGE
    # a segment made only of such rows is a segment without rows
    got = R.segment_boxes(np.full((4, 3), np.nan, np.float32), np.zeros(4, np.int32), 1, T)
    assert got["err"] == R.ERR_NONFINITE and got["angle"][0] == -1 and got["n"][0] == 0 and not u32(got["center"]).any()


def test_helpers_on_hand_made_boxes():
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    b = boxes.Boxes(f([[1.0, 2.0, 0.5], [0.0, 0.0, 0.0]]), f([[2.0, 4.0, 1.0], [4.0, 2.0, 2.0]]), f([0.25, math.pi / 4]),
                    torch.tensor([3, 32], dtype=torch.int32), f([[0, 0, 0], [0, 0, 0]]), f([[0, 0, 0], [0, 0, 0]]),
                    torch.tensor([5, 6], dtype=torch.int32), torch.tensor([7, 8], dtype=torch.int64))
    c = boxes.canonical(b)
    assert c.size.tolist() == [[4.0, 2.0, 1.0], [4.0, 2.0, 2.0]]
    assert abs(float(c.yaw[0]) - (0.25 + math.pi / 2)) < 1e-6 and float(c.yaw[1]) == float(b.yaw[1]) and (c.yaw >= 0).all() and (c.yaw < math.pi).all()
    assert torch.equal(c.center, b.center) and torch.equal(c.angle, b.angle) and torch.equal(c.n, b.n) and torch.equal(c.score, b.score)
    k = boxes.corners(b)
    assert k.shape == (2, 8, 3)
    assert torch.allclose(k.mean(1), b.center, atol=1e-6)
    assert torch.allclose(k[1, :4, 2], f([-1.0] * 4)) and torch.allclose(k[1, 4:, 2], f([1.0] * 4))
    r = math.sqrt(2.0)                                               # a 4 x 2 box turned by 45 degrees about the origin
    want = f([[-r / 2, -3 * r / 2], [3 * r / 2, r / 2], [-3 * r / 2, -r / 2], [r / 2, 3 * r / 2]])
    assert torch.allclose(k[1, :4, :2], want, atol=1e-6)
    assert torch.allclose(boxes.corners(c)[0].sort(0).values, k[0].sort(0).values, atol=1e-5)            # the same eight corners
    pts = f([[r, r, 0.0, 9.0], [r, r, 1.5, 9.0], [1.6 * r, 1.6 * r, 0.0, 9.0], [0.0, 0.0, 0.0, 9.0], [1.0, 2.0, 0.5, 9.0], [1.0, 4.5, 0.5, 9.0]])
    ids = torch.tensor([1, 1, 1, -1, 0, 0], dtype=torch.int32)
    assert boxes.contains(b, pts, ids).tolist() == [True, False, False, False, True, False]
    assert boxes.contains(b, pts, ids, margin=0.6).tolist() == [True, True, False, False, True, True]
    assert boxes.contains(c, pts, ids).tolist() == boxes.contains(b, pts, ids).tolist()
    assert np.array_equal(u32(boxes.angle_table_np(90)), u32(R.angle_table(90)))
    with pytest.raises(ValueError):
        boxes.angle_table_np(257)


def test_binding_header_and_build_agree():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+15\b", text) and _lib.ABI_VERSION == 15          # added within the ABI
    for name, value in (("PN2_BOX_ERR_RANGE", _lib.BOX_ERR_RANGE), ("PN2_BOX_ERR_NONFINITE", _lib.BOX_ERR_NONFINITE),
                        ("PN2_BOX_MAX_ANGLES", _lib.BOX_MAX_ANGLES)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert (R.ERR_RANGE, R.ERR_NONFINITE) == (_lib.BOX_ERR_RANGE, _lib.BOX_ERR_NONFINITE)
    others = [_lib.VOXEL_ERR_RANGE, _lib.VOXEL_ERR_ROWS, _lib.SEGMENT_ERR_RANGE, _lib.SEGMENT_ERR_NONFINITE, _lib.CLUSTER_ERR_INDEX,
              _lib.CLUSTER_ERR_CELL, _lib.CLUSTER_ERR_CAP, _lib.CLUSTER_ERR_ROWS, _lib.PANOPTIC_ERR_CLASS, _lib.PANOPTIC_ERR_ROWS]
    bits = others + [_lib.BOX_ERR_RANGE, _lib.BOX_ERR_NONFINITE]
    assert sum(bits) == np.bitwise_or.reduce(bits) and all(b & (b - 1) == 0 for b in bits)            # disjoint single bits
    lib = _lib.load()
    assert len(_lib.SIGNATURES["pn2_segment_boxes"][1]) == 27 and hasattr(lib, "pn2_segment_boxes")
    assert lib.pn2_segment_boxes_workspace_bytes(1, 0) == 16 and lib.pn2_segment_boxes_workspace_bytes(3, 1000) == 4 * 12000 + 16
    for B, rows in ((0, 10), (65536, 10), (1, -1), (1, (1 << 29) + 1)):
        assert lib.pn2_segment_boxes_workspace_bytes(B, rows) == -1
    assert lib.pn2_segment_boxes(None, 3, 0, 1, 2, None, None, None, 1, 0, None, None, None, 1, 0.05, 0, None, None, None, None, None, None,
                                 None, None, None, None, None) == -1             # null pointers: refused on the host, no GPU needed
    with pytest.raises(_lib.Pn2Error):
        boxes.segment_boxes(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), 1)
    make = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert re.search(r"^boxes\.o:.*\n\t.*-ffp-contract=off", make, re.M) and " boxes.o " in make


def test_generated_code_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "boxes.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
