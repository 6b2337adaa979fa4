"""CPU: the yardsticks of the 3-D ego view (tests/view3d_ref.py) agree with each other, and the open3d file parsers of
pointnet12_amd/kitti_view.py return the numbers of the reference's own settings (tests/golden/g19_ego_view.npz)."""
import json

import numpy as np
import pytest

from conftest import golden
import view3d_ref as VR

from pointnet12_amd import kitti_view as V

SIZES = [(53, 37), (800, 800)]                             # (W, H)
COUNTS = [0, 1, 63, 64, 65, 257, 2048]
POINT_SIZES = [1, 2, 3, 5]


def fixture_camera():
    g = golden("g19_ego_view.npz")
    cam = VR.Camera(g["extrinsic"].reshape(4, 4).T[:3], g["intrinsic_matrix"].reshape(3, 3).T[[0, 1, 0, 1], [0, 1, 2, 2]],
                    int(g["width"]), int(g["height"]))
    return g, cam


@pytest.mark.parametrize("size", SIZES)
def test_the_two_statements_agree_byte_for_byte(size):
    W, H = size
    cam = VR.unit_camera(W, H)
    for N in COUNTS:
        pts = VR.cloud(N, W, H)
        for s in POINT_SIZES:
            depth, index = VR.reference(N, W, H, s)
            depth2, index2 = VR.per_pixel(pts, cam, s, VR.NEAR, VR.FAR)
            assert np.array_equal(depth.view(np.uint32), depth2.view(np.uint32)), (N, s)
            assert np.array_equal(index, index2), (N, s)
            assert ((index >= 0) == np.isfinite(depth)).all()
            if N >= 257:
                missing = [k for k, v in VR.occurred(pts, cam, s, VR.NEAR, VR.FAR).items() if not v]
                assert not missing, (N, s, missing)
                assert (index >= 0).sum() > 100
    assert (VR.reference(0, W, H, 2)[1] == -1).all()


def test_the_planted_rules_decide_as_stated():
    """The painter on hand-checked pixels of the 37 x 53 case: who must be visible where, written out."""
    W, H = 53, 37
    cam = VR.unit_camera(W, H)
    n = len(VR.planted(W, H))                                   # the planted points alone
    pts = VR.cloud(n, W, H)
    drawn, d, xw, yw, Z = VR.project(pts, cam, VR.NEAR, VR.FAR)
    depth, index = VR.reference(n, W, H, 1)
    assert index[10, 10] == 1 and depth[10, 10] == 2.0          # the nearer point came second
    assert index[10, 20] == 2 and depth[10, 20] == 2.0          # ... and first
    assert index[10, 30] == 4                                   # three duplicates: the lowest index
    assert index[10, 40] == 7 and d[7] == d[8] and Z[8] < Z[7]  # one float32 depth: the index decides, not the fp64 depth
    assert not drawn[9:19].any() and drawn[19] and drawn[20]    # near, below it, negative, zero, NaN, inf, far and beyond
    assert xw[39] == 7.0 and xw[40] == 7.5 and yw[46] == 20.0 and yw[47] == 20.5
    for s, cols7, cols75 in ((1, [7], [7]), (2, [6, 7], [7, 8]), (3, [6, 7, 8], [6, 7, 8]), (5, [5, 6, 7, 8, 9], [5, 6, 7, 8, 9])):
        _, idx = VR.paint(pts[[39]], cam, s, VR.NEAR, VR.FAR)   # a centre on k = 7: where the floor rule flips for even sizes
        assert sorted(set(np.nonzero(idx >= 0)[1].tolist())) == cols7, s
        _, idx = VR.paint(pts[[40]], cam, s, VR.NEAR, VR.FAR)   # ... and on k + 0.5
        assert sorted(set(np.nonzero(idx >= 0)[1].tolist())) == cols75, s


def test_colour_and_the_error_flag():
    index = np.array([[-1, 0], [2, 1]], np.int32)
    colors = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    img, err = VR.colour(index, [1, 0, 1], colors, (9, 8, 7))
    assert err == 0 and img.tolist() == [[[9, 8, 7], [4, 5, 6]], [[4, 5, 6], [1, 2, 3]]]
    img, err = VR.colour(index, [1, 2, -1], colors, (9, 8, 7))
    assert err == 1 and img.tolist() == [[[9, 8, 7], [4, 5, 6]], [[9, 8, 7], [9, 8, 7]]]


# ------------------------------------------------------------------------------------------------------------------ parsers
def write_camera(path, g, extra=True):
    d = {"class_name": "PinholeCameraParameters", "extrinsic": g["extrinsic"].tolist(),
         "intrinsic": {"height": int(g["height"]), "intrinsic_matrix": g["intrinsic_matrix"].tolist(), "width": int(g["width"])},
         "version_major": 1, "version_minor": 0}
    if extra:
        d.update({"h_fov": [-40, 40], "v_fov": [-20, 20], "x_range": None, "d_range": [0, 80], "something_else": {"a": [1, 2]}})
    path.write_text(json.dumps(d, indent=4))
    return str(path)


def write_option(path, g, **over):
    d = {"background_color": g["background_color"].tolist(), "class_name": "RenderOption", "point_size": float(g["point_size"]),
         "light_on": True, "line_width": 1.0, "light0_position": [0.0, 0.0, 2.0], "version_major": 1}
    d.update(over)
    path.write_text(json.dumps(d, indent=4))
    return str(path)


def test_camera_from_json_returns_the_fixtures_numbers(tmp_path):
    g = golden("g19_ego_view.npz")
    cam = V.PinholeCamera.from_json(write_camera(tmp_path / "ego_view.json", g))
    assert (cam.width, cam.height) == (800, 800) == (int(g["width"]), int(g["height"]))
    assert cam.extrinsic.dtype == np.float64 and cam.extrinsic.shape == (4, 4) and cam.intrinsic.shape == (3, 3)
    assert np.array_equal(cam.extrinsic, g["extrinsic"].reshape(4, 4).T)                # column-major
    assert np.array_equal(cam.extrinsic[:3, 3], g["extrinsic"][12:15]) and np.array_equal(cam.extrinsic[3], [0, 0, 0, 1])
    assert cam.E.shape == (3, 4) and cam.E.flags.c_contiguous and np.array_equal(cam.E, cam.extrinsic[:3])
    assert cam.E[2].tolist() == [0.9183303370700582, 0.06773143291149537, -0.38997672368046415, 18.14031098830259]
    assert np.array_equal(cam.intrinsic, g["intrinsic_matrix"].reshape(3, 3).T)
    assert cam.K.tolist() == [692.820323027551, 692.820323027551, 399.5, 399.5]
    bare = V.PinholeCamera.from_json(write_camera(tmp_path / "bare.json", g, extra=False))  # unknown keys change nothing
    assert np.array_equal(bare.extrinsic, cam.extrinsic) and np.array_equal(bare.K, cam.K)
    direct = V.PinholeCamera(cam.extrinsic, cam.intrinsic, 800, 800)
    assert np.array_equal(direct.E, cam.E) and np.array_equal(direct.K, cam.K)
    with pytest.raises(ValueError):
        V.PinholeCamera(cam.extrinsic, [[1, 0.5, 0], [0, 1, 0], [0, 0, 1]], 8, 8)        # a skewed camera is refused
    bad = json.loads(open(tmp_path / "bare.json").read())
    bad["extrinsic"] = bad["extrinsic"][:12]
    (tmp_path / "bad.json").write_text(json.dumps(bad))
    with pytest.raises(ValueError):
        V.PinholeCamera.from_json(str(tmp_path / "bad.json"))


def test_render_option_from_json(tmp_path):
    g = golden("g19_ego_view.npz")
    opt = V.RenderOption.from_json(write_option(tmp_path / "render_option.json", g))
    assert opt.point_size == 2 == g["point_size"] and isinstance(opt.point_size, int)
    assert opt.background_color == (0, 0, 0) == tuple(int(round(c * 255)) for c in g["background_color"])
    opt = V.RenderOption.from_json(write_option(tmp_path / "b.json", g, point_size=5.0, background_color=[1.0, 0.5, 0.2]))
    assert opt.point_size == 5 and opt.background_color == (255, round(0.5 * 255), 51)
    with pytest.raises(ValueError):
        V.RenderOption.from_json(write_option(tmp_path / "c.json", g, point_size=2.5))
    with pytest.raises(ValueError):
        V.RenderOption.from_json(write_option(tmp_path / "d.json", g, background_color=[0.0, 2.0, 0.0]))
    (tmp_path / "e.json").write_text("{}")                                               # missing keys: the package's defaults
    opt = V.RenderOption.from_json(str(tmp_path / "e.json"))
    assert opt.point_size == 2 and opt.background_color == (0, 0, 0)


def test_render_points_refuses_cpu_tensors():
    import torch
    from pointnet12_amd import _lib
    g, _ = fixture_camera()
    cam = V.PinholeCamera(g["extrinsic"].reshape(4, 4).T, g["intrinsic_matrix"].reshape(3, 3).T, 800, 800)
    with pytest.raises(_lib.Pn2Error):
        V.render_points(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), np.zeros((2, 3), np.uint8), cam)


def test_argument_checks_need_no_gpu():
    import ctypes
    from pointnet12_amd import _lib
    lib = _lib.load()
    E = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2)
    K = (ctypes.c_double * 4)(16, 16, -0.5, -0.5)
    fake = ctypes.c_void_p(4096)                                                         # never dereferenced: every call is refused
    call = lambda **k: lib.pn2_depth_splat(k.get("xyz", fake), k.get("ldx", 3), k.get("N", 4), E, K, k.get("near", 0.1),
                                           k.get("far", 1000.0), k.get("s", 2), k.get("H", 8), k.get("W", 8), k.get("zkey", fake), None)
    assert call(s=17) == _lib.PN2_EUNSUPPORTED and call(s=0) == _lib.PN2_EUNSUPPORTED
    for bad in (dict(near=1.0, far=1.0), dict(near=2.0, far=1.0), dict(near=0.0), dict(near=-1.0), dict(far=3.1e38),
                dict(near=float("nan")), dict(far=float("nan")), dict(ldx=2), dict(N=-1), dict(N=2 ** 31), dict(zkey=None),
                dict(xyz=None), dict(H=0), dict(W=-3), dict(H=65536, W=32768)):
        assert call(**bad) == -1, bad
    assert lib.pn2_depth_resolve(None, 8, 8, fake, fake, None) == -1
    assert lib.pn2_depth_resolve(fake, 65536, 32768, fake, fake, None) == -1
