#!/usr/bin/env python3
"""Generate tests/golden/g19_ego_view.npz (development container only): the settings of the reference's 3-D ego view.

Stored, and nothing else: the 16 ``extrinsic`` numbers, the 9 ``intrinsic.intrinsic_matrix`` numbers (both in the file's own
COLUMN-major order), ``width`` and ``height`` of the reference's ``config/ego_view.json`` (an open3d ``PinholeCameraParameters``
file, read by ``Window_Manager.__init__``, pcdvis.py:33), and ``point_size`` and ``background_color`` of its
``config/render_option.json`` (:37).  ``PinholeCamera.from_json`` / ``RenderOption.from_json`` of pointnet12_amd/kitti_view.py are
run on the two files while doing so and must return the same numbers.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_view3d.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PN2_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from pointnet12_amd import kitti_view as V       # noqa: E402


def main():
    fn_cam, fn_opt = os.path.join(REF, "config", "ego_view.json"), os.path.join(REF, "config", "render_option.json")
    cam, opt = json.load(open(fn_cam)), json.load(open(fn_opt))
    out = {"extrinsic": np.array(cam["extrinsic"], np.float64), "intrinsic_matrix": np.array(cam["intrinsic"]["intrinsic_matrix"], np.float64),
           "width": np.int64(cam["intrinsic"]["width"]), "height": np.int64(cam["intrinsic"]["height"]),
           "point_size": np.float64(opt["point_size"]), "background_color": np.array(opt["background_color"], np.float64)}
    assert out["extrinsic"].shape == (16,) and out["intrinsic_matrix"].shape == (9,) and out["background_color"].shape == (3,)
    mine = V.PinholeCamera.from_json(fn_cam)
    assert (mine.extrinsic == out["extrinsic"].reshape(4, 4).T).all() and (mine.intrinsic == out["intrinsic_matrix"].reshape(3, 3).T).all()
    assert (mine.width, mine.height) == (int(out["width"]), int(out["height"]))
    assert (mine.E[:, 3] == out["extrinsic"][12:15]).all()                   # column-major: the translation is numbers 12 .. 14
    ro = V.RenderOption.from_json(fn_opt)
    assert ro.point_size == out["point_size"] and ro.background_color == tuple(int(round(c * 255)) for c in out["background_color"])
    print("  ok: camera %d x %d, fx %.6f, E[2] = %s; point size %d, background %s"
          % (mine.width, mine.height, mine.K[0], mine.E[2].tolist(), ro.point_size, ro.background_color))
    path = os.path.join(ROOT, "tests", "golden", "g19_ego_view.npz")
    np.savez_compressed(path, **out)
    np.load(path, allow_pickle=False)["extrinsic"]
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
