"""CPU: what of the KITTI frame path (pointnet12_amd/kitti_view.py, csrc/view.hip) needs no device.  The calibration parsers, the
class tables and the merge tables are held to what the reference's own code returned (tests/golden/g18_kitti_view.npz,
tools/make_golden_kitti_view.py), and so is the projection restatement the GPU tests use as their yardstick."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import kitti_view_ref as KR

from pointnet12_amd import _lib
from pointnet12_amd import kitti_view as V


def G():
    return golden("g18_kitti_view.npz")


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def config(g):
    return {name: dict(zip(g[name + "_keys"].tolist(), g[name + "_values"].tolist()))
            for name in ("labels", "color_map", "learning_map_inv")}


def test_calibration_parsers_reproduce_the_reference_bit_for_bit(tmp_path):
    g = G()
    fv, fc = tmp_path / "calib_velo_to_cam.txt", tmp_path / "calib_cam_to_cam.txt"
    fv.write_text(str(g["calib_velo_to_cam_txt"]))
    fc.write_text(str(g["calib_cam_to_cam_txt"]))
    R, T = V.calib_velo2cam(str(fv))
    P = V.calib_cam2cam(str(fc), mode="02")
    for mine, ref in ((R, g["R"]), (T, g["T"]), (P, g["P"])):
        assert mine.dtype == np.float64 and mine.shape == ref.shape and (bits64(mine) == bits64(ref)).all()
    calib = V.Calibration(R, T, P)
    assert calib.RT.shape == (3, 4) and (bits64(calib.RT) == bits64(np.concatenate((g["R"], g["T"]), axis=1))).all()
    assert (bits64(V.Calibration.from_files(str(fv), str(fc)).RT) == bits64(calib.RT)).all()
    assert V.calib_cam2cam(str(fc), mode="00").shape == (3, 3)
    with pytest.raises(ValueError):
        V.calib_cam2cam(str(fv))


def test_classes_from_config_equal_the_reference_tables():
    g = G()
    names, colors, bgr = V.classes_from_config(config(g))
    assert names == g["class_names"].tolist() and len(names) == 19
    assert colors.dtype == np.uint8 and colors.shape == (19, 3) and (colors == g["colors"]).all()
    assert bgr.dtype == np.uint8 and (bgr == g["colors"][:, ::-1]).all()


def test_merge_groups_on_both_recorded_lists():
    g = G()
    for names, merged, colors in ((g["class_names"].tolist(), g["merge_semkitti"].tolist(), g["colors"]),
                                  (g["kitti_class_names"].tolist(), g["merge_kitti"].tolist(), g["kitti_colors"])):
        t = V.merge_groups(names, merged, colors)
        assert len(t) == len(merged) == 16 and t.begin.dtype == np.int32 and t.member.dtype == np.int32
        assert t.begin[0] == 0 and t.begin[-1] == len(t.member) == 19
        for k, entry in enumerate(merged):
            assert t.members(k) == [names.index(p) for p in entry.split("+")]
            assert (t.colors[k] == colors[names.index(entry.split("+")[0])]).all()
        assert sorted(t.member.tolist()) == list(range(19))
    names = g["class_names"].tolist()
    three = V.merge_groups(names, ["car+truck+other-vehicle", "road"])
    assert three.members(0) == [names.index("car"), names.index("truck"), names.index("other-vehicle")] and three.colors is None
    with pytest.raises(ValueError):
        V.merge_groups(names, ["road", "parking+pavement"])


def test_projection_restatement_equals_the_reference_output_bit_for_bit():
    g = G()
    RT = np.concatenate((g["R"], g["T"]), axis=1)
    mine, ref = KR.project(g["points"], RT, g["P"]), g["pts_2d"]
    assert mine.dtype == np.float32 and mine.shape == ref.shape == (2048, 2)
    assert ((mine.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(mine) & np.isnan(ref))).all()
    big = np.abs(ref.astype(np.float64)) >= 2.0 ** 31                       # the camera-plane point is in the fixture
    assert big.any() and (KR.pixels(ref)[big.any(1)] == KR.INT32_MIN).all()
    near = np.abs(ref[-8:].astype(np.float64) - np.round(ref[-8:].astype(np.float64))).min(1)
    assert (near < 1e-3).all()                                              # ... and so are the near-integer pixels


def test_cpu_tensors_and_missing_disc_tables_are_refused():
    lp = torch.zeros(4, 19)
    with pytest.raises(_lib.Pn2Error):
        V.predict(lp)
    with pytest.raises(_lib.Pn2Error):
        V.merge_classes(lp, V.Groups([0, 1], [0]))
    with pytest.raises(_lib.Pn2Error):
        V.draw_2d_points(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), np.zeros((19, 3), np.uint8))
    with pytest.raises(_lib.Pn2Error):
        V.project_3d_to_2d(torch.zeros(4, 3), V.Calibration(np.eye(3), np.zeros((3, 1)), np.eye(3)))
    assert sorted(V.DISC_HALF_WIDTHS) == [2, 3]
    assert sum(2 * h + 1 for h in V.DISC_HALF_WIDTHS[2]) == 21 and sum(2 * h + 1 for h in V.DISC_HALF_WIDTHS[3]) == 37
    with pytest.raises(ValueError):
        V._half_widths(4, None)
    assert V._half_widths(4, [0, 1, 2, 3, 4, 3, 2, 1, 0])[1].tolist() == [0, 1, 2, 3, 4, 3, 2, 1, 0]
    with pytest.raises(ValueError):
        V._half_widths(2, [1, 2, 1])
    assert "UNVERIFIED AGAINST OPENCV" in V.__doc__
    assert V.torch_project_3d_to_2d is V.project_3d_to_2d


def test_entry_points_are_declared_bound_exported_and_check_their_arguments_on_the_host():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    lib = _lib.load()
    for name, nargs in (("pn2_seg_predict", 11), ("pn2_project_points", 8), ("pn2_splat_discs", 8), ("pn2_splat_resolve", 11)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
        assert len(_lib.SIGNATURES[name][1]) == nargs and hasattr(lib, name)
    one = ctypes.c_void_p(256)                                  # a non-NULL placeholder: refused calls launch nothing
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    # predict: pitch below C, too many classes, group tables that are empty / out of range / unsorted; R == 0 is a no-op
    assert lib.pn2_seg_predict(None, 20, 8, 19, None, None, 0, one, None, 0, None) == -1
    assert lib.pn2_seg_predict(one, 16, 8, 19, None, None, 0, one, None, 0, None) == -1
    assert lib.pn2_seg_predict(one, 68, 8, 65, None, None, 0, one, None, 0, None) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_seg_predict(one, 20, 8, 19, None, None, 0, one, one, 4, None) == -1          # merged without groups
    assert lib.pn2_seg_predict(one, 20, 8, 19, i32(0, 1, 1), i32(3), 2, one, None, 0, None) == -1
    assert lib.pn2_seg_predict(one, 20, 8, 19, i32(0, 1, 2), i32(3, 19), 2, one, None, 0, None) == -1
    assert lib.pn2_seg_predict(one, 20, 8, 19, i32(0, 1, 2), i32(3, -1), 2, one, None, 0, None) == -1
    assert lib.pn2_seg_predict(one, 20, 8, 19, i32(1, 2, 3), i32(3, 4, 5), 2, one, None, 0, None) == -1
    assert lib.pn2_seg_predict(one, 20, 8, 19, i32(0, 1, 2), i32(3, 4), 2, one, one, 1, None) == -1      # ldm below G
    assert lib.pn2_seg_predict(one, 20, 0, 19, i32(0, 1, 2), i32(3, 4), 2, one, one, 2, None) == 0
    assert lib.pn2_seg_predict(one, 20, 0, 19, None, None, 0, one, None, 0, None) == 0
    # project: pitch below 3, one matrix without the other, nothing to write; N == 0 is a no-op
    d = (ctypes.c_double * 12)()
    assert lib.pn2_project_points(one, 2, 8, d, d, one, None, None) == -1
    assert lib.pn2_project_points(one, 3, 8, d, None, one, None, None) == -1
    assert lib.pn2_project_points(one, 3, 8, d, d, None, None, None) == -1
    assert lib.pn2_project_points(one, 3, 8, None, None, one, one, None) == -1
    assert lib.pn2_project_points(one, 3, 0, d, d, one, one, None) == 0
    assert lib.pn2_project_points(one, 4, 0, None, None, None, one, None) == 0
    # splat: image sizes, radius, table entries
    assert lib.pn2_splat_discs(one, 8, i32(1, 2, 2, 2, 1), 2, 0, 64, one, None) == -1
    assert lib.pn2_splat_discs(one, 8, i32(1, 2, 2, 2, 1), 2, 65536, 65536, one, None) == -1
    assert lib.pn2_splat_discs(one, 8, None, 2, 48, 64, one, None) == -1
    assert lib.pn2_splat_discs(one, 8, i32(1, 2, -2, 2, 1), 2, 48, 64, one, None) == -1
    assert lib.pn2_splat_discs(one, 8, i32(*([1] * 67)), 33, 48, 64, one, None) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_splat_discs(None, 8, i32(1, 2, 2, 2, 1), 2, 48, 64, one, None) == -1
    assert lib.pn2_splat_resolve(None, 48, 64, one, 8, one, 19, None, one, None, None) == -1
    assert lib.pn2_splat_resolve(one, 48, 64, None, 8, one, 19, None, one, None, None) == -1
    assert lib.pn2_splat_resolve(one, 48, 64, one, 8, one, 19, None, None, None, None) == -1
    assert lib.pn2_splat_resolve(one, 48, 0, one, 8, one, 19, None, one, None, None) == -1
