#!/usr/bin/env python3
"""Generate tests/golden/g18_kitti_view.npz (development container only): the reference's own calibration parsers and
``project_3d_to_2d`` on its own calibration files, and its class tables.

``data_utils/kitti_utils.py`` cannot be imported here (cv2), so ``calib_velo2cam``, ``calib_cam2cam`` and ``project_3d_to_2d`` of
``Semantic_KITTI_Utils`` are compiled from the reference file's own syntax tree into a bare class and run unmodified; its
module-level tables (``sem_kitti_class_names``, ``sem_kitti_colors``) and the merge lists of ``KITTI_2_Common`` /
``SemKITTI_2_Common`` are literal-evaluated from the same tree.  Stored: the text of the two calibration files (settings only),
the parsed R, T, P, 2 048 points with what the reference returned for them, the tables, and the ``labels`` / ``color_map`` /
``learning_map_inv`` blocks of the reference's ``config/semantic-kitti.yaml``.  pointnet12_amd/kitti_view.py (parsers, class
tables, merge tables) and tests/kitti_view_ref.py (the projection) are asserted bit-equal while doing so.

The points: x uniform in 0.5 .. 70, y in +-40, z in +-3; 64 points with x in -5 .. 0.3 (behind and around the camera plane);
one point ON the camera plane (c_2 == 0 in float32 if the search finds one, else the nearest); 8 points whose pixel lands within
1e-3 of an integer.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_kitti_view.py
"""
import ast
import os
import sys
import tempfile
import warnings

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PN2_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kitti_view_ref as KR                      # noqa: E402
from pointnet12_amd import kitti_view as V       # noqa: E402

WANT = ("calib_velo2cam", "calib_cam2cam", "project_3d_to_2d")


def reference_tree():
    path = os.path.join(REF, "data_utils", "kitti_utils.py")
    return path, ast.parse(open(path).read(), path)


def reference_utils(path, tree):
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Semantic_KITTI_Utils"][0]
    cls.body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert len(cls.body) == len(WANT)
    ns = {"np": np, "os": os}
    exec(compile(ast.Module(body=[cls], type_ignores=[]), path, "exec"), ns)
    return ns["Semantic_KITTI_Utils"]


def module_literal(tree, name):
    for n in tree.body:
        if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == name:
            return ast.literal_eval(n.value)
    raise KeyError(name)


def init_literal(tree, cls_name, attr):
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name][0]
    init = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"][0]
    for n in init.body:
        if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Attribute) and n.targets[0].attr == attr:
            return ast.literal_eval(n.value)
    raise KeyError(attr)


def camera_plane_point(RT):
    """An fp32 point whose camera depth c_2 rounds to exactly 0 in float32 if the search meets one, else the smallest |c_2|."""
    best = None
    for y in np.float32([0.0, 0.5, -1.25, 3.0]):
        for z in np.float32([0.0, -1.0, 0.75, 1.5]):
            x0 = np.float32(-(RT[2, 1] * float(y) + RT[2, 2] * float(z) + RT[2, 3]) / RT[2, 0])
            xs = x0.view(np.uint32) + np.arange(-4096, 4097, dtype=np.int64)
            xs = xs.astype(np.uint32).view(np.float32)
            c2 = (((RT[2, 0] * xs.astype(np.float64) + RT[2, 1] * float(y)) + RT[2, 2] * float(z)) + RT[2, 3] * 1.0).astype(np.float32)
            k = int(np.argmin(np.abs(c2)))
            if best is None or abs(c2[k]) < best[0]:
                best = (abs(float(c2[k])), np.float32([xs[k], y, z]))
    return best


def near_integer_points(rng, RT, P, count=8):
    out = []
    want = [(0, +1), (0, -1), (1, +1), (1, -1)] * (count // 4)        # (component, side of the integer)
    while want:
        cand = np.stack([rng.uniform(3, 60, 400000), rng.uniform(-20, 20, 400000), rng.uniform(-2, 1, 400000)], 1).astype(np.float32)
        uv = KR.project(cand, RT, P).astype(np.float64)
        for comp, side in list(want):
            d = uv[:, comp] - np.round(uv[:, comp])
            hit = np.nonzero((d * side > 0) & (np.abs(d) < 1e-3) & (uv[:, 0] > 0) & (uv[:, 0] < 1242) & (uv[:, 1] > 0) & (uv[:, 1] < 375))[0]
            if len(hit):
                out.append(cand[hit[0]])
                want.remove((comp, side))
    return np.stack(out)


def main():
    path, tree = reference_tree()
    Utils = reference_utils(path, tree)
    fv, fc = os.path.join(REF, "config", "calib_velo_to_cam.txt"), os.path.join(REF, "config", "calib_cam_to_cam.txt")
    u = Utils.__new__(Utils)                                 # no __init__: it needs cv2 objects and a dataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)  # (the reference parses with np.fromstring)
        R, T = u.calib_velo2cam(fv)
        P = u.calib_cam2cam(fc, mode="02")
    u.R, u.T, u.P = R, T, P
    u.RT = np.concatenate((R, T), axis=1)
    text_v, text_c = open(fv).read(), open(fc).read()
    with tempfile.TemporaryDirectory() as tmp:               # the module's parsers, from the RECORDED texts
        a, b = os.path.join(tmp, "v.txt"), os.path.join(tmp, "c.txt")
        open(a, "w").write(text_v)
        open(b, "w").write(text_c)
        calib = V.Calibration.from_files(a, b)
    for mine, ref in ((calib.R, R), (calib.T, T), (calib.P, P), (calib.RT, u.RT)):
        assert mine.shape == ref.shape and (mine.view(np.uint64) == np.ascontiguousarray(ref).view(np.uint64)).all()

    rng = np.random.default_rng(2026)
    n_main = 2048 - 64 - 1 - 8
    main_pts = np.stack([rng.uniform(0.5, 70, n_main), rng.uniform(-40, 40, n_main), rng.uniform(-3, 3, n_main)], 1)
    behind = np.stack([rng.uniform(-5, 0.3, 64), rng.uniform(-40, 40, 64), rng.uniform(-3, 3, 64)], 1)
    c2, plane = camera_plane_point(u.RT)
    near = near_integer_points(rng, u.RT, P)
    pts = np.concatenate([main_pts, behind, plane[None], near], 0).astype(np.float32)
    assert pts.shape == (2048, 3)
    with np.errstate(all="ignore"):
        ref2d = u.project_3d_to_2d(pts)
    assert ref2d.dtype == np.float32 and ref2d.shape == (2048, 2)
    mine2d = KR.project(pts, u.RT, P)
    same = (ref2d.view(np.uint32) == mine2d.view(np.uint32)) | (np.isnan(ref2d) & np.isnan(mine2d))
    assert same.all(), "tests/kitti_view_ref.project differs from the reference in %d floats" % (~same).sum()
    print("  ok: projection restatement bit-equal on %d points; camera-plane |c_2| = %g -> %s; %d non-finite results"
          % (len(pts), c2, ref2d[n_main + 64], (~np.isfinite(ref2d)).any(1).sum()))

    names = module_literal(tree, "sem_kitti_class_names")
    colors = np.array(module_literal(tree, "sem_kitti_colors"), np.uint8)
    merge_sem = init_literal(tree, "SemKITTI_2_Common", "semkitti_2_common")
    merge_kitti = init_literal(tree, "KITTI_2_Common", "kitti_2_common")
    kitti_names = module_literal(tree, "kitti_class_names")
    kitti_colors = np.array(module_literal(tree, "kitti_colors"), np.uint8)
    cfg = yaml.safe_load(open(os.path.join(REF, "config", "semantic-kitti.yaml")))
    my_names, my_colors, my_bgr = V.classes_from_config(cfg)
    assert my_names == names and (my_colors == colors).all() and (my_bgr == colors[:, ::-1]).all()
    for nm, lst, col in ((names, merge_sem, colors), (kitti_names, merge_kitti, kitti_colors)):
        g = V.merge_groups(nm, lst, col)
        for k, entry in enumerate(lst):
            assert g.members(k) == [nm.index(p) for p in entry.split("+")]
            assert (g.colors[k] == col[nm.index(entry.split("+")[0])]).all()
    print("  ok: class tables from the yaml and both merge tables equal the reference's")

    def block(name):
        keys = np.array(sorted(cfg[name]), np.int64)
        return keys, [cfg[name][int(k)] for k in keys]

    lk, lv = block("labels")
    ck, cv = block("color_map")
    ik, iv = block("learning_map_inv")
    out = {"calib_velo_to_cam_txt": np.array(text_v), "calib_cam_to_cam_txt": np.array(text_c), "R": R, "T": T, "P": P,
           "points": pts, "pts_2d": ref2d, "class_names": np.array(names), "colors": colors,
           "kitti_class_names": np.array(kitti_names), "kitti_colors": kitti_colors,
           "merge_semkitti": np.array(merge_sem), "merge_kitti": np.array(merge_kitti),
           "labels_keys": lk, "labels_values": np.array(lv), "color_map_keys": ck, "color_map_values": np.array(cv, np.int64),
           "learning_map_inv_keys": ik, "learning_map_inv_values": np.array(iv, np.int64)}
    path = os.path.join(ROOT, "tests", "golden", "g18_kitti_view.npz")
    np.savez_compressed(path, **out)
    np.load(path, allow_pickle=False)["class_names"]
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
