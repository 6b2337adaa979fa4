"""GPU: the 3-D ego view (``render_points`` of pointnet12_amd/kitti_view.py on ``pn2_depth_splat`` / ``pn2_depth_resolve`` of
csrc/view.hip).

Every image, depth map and index map is held BYTE FOR BYTE to the fp64 restatement of tests/view3d_ref.py (its sequential
painter; tests/test_ego_view_cpu.py holds that painter to an independent per-pixel statement): no tolerance, no excluded pixel.
The rule is the one include/pn2.h states; it is not checked against open3d, which is not available.  Shapes are the smallest that
reach every path: a 37 x 53 image (no multiple of the 256-thread block) and the reference camera's 800 x 800, point counts around
the 64-lane wave and past one block, point sizes of both parities."""
import json

import numpy as np
import pytest
import torch

from conftest import golden
import kitti_view_ref as KR
import view3d_ref as VR

from pointnet12_amd import _lib
from pointnet12_amd import kitti_view as V
from pointnet12_amd import synthetic as syn

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 257, 2048]
POINT_SIZES = [1, 2, 3, 5]


def camera_of(ref_cam):
    ext = np.concatenate([ref_cam.E, [[0.0, 0.0, 0.0, 1.0]]], 0)
    fx, fy, cx, cy = ref_cam.K
    return V.PinholeCamera(ext, [[fx, 0, cx], [0, fy, cy], [0, 0, 1]], ref_cam.width, ref_cam.height)


def fixture_cameras():
    g = golden("g19_ego_view.npz")
    cam = V.PinholeCamera(g["extrinsic"].reshape(4, 4).T, g["intrinsic_matrix"].reshape(3, 3).T, int(g["width"]), int(g["height"]))
    return cam, VR.Camera(cam.E, cam.K, cam.width, cam.height), int(g["point_size"])


def palette(C=19, seed=0):
    return np.random.default_rng(seed).integers(1, 256, size=(C, 3)).astype(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def same_tensor(a, b):
    """``torch.equal`` on the bytes (a depth map holds +inf; bit patterns are what is promised)."""
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("size", [(53, 37), (800, 800)])
def test_image_depth_and_index_are_the_restatement_byte_for_byte(dev, size):
    W, H = size
    ref_cam = VR.unit_camera(W, H)
    cam = camera_of(ref_cam)
    colors = palette()
    for N in COUNTS:
        pts = VR.cloud(N, W, H)
        labels = np.random.default_rng(N).integers(0, 19, N).astype(np.int64)
        x, l = torch.from_numpy(pts.copy()).to(dev), torch.from_numpy(labels).to(dev)
        for s in POINT_SIZES:
            if N >= 257:                                   # the planted cases are in the input before anything is compared
                missing = [k for k, v in VR.occurred(pts, ref_cam, s, VR.NEAR, VR.FAR).items() if not v]
                assert not missing, (N, s, missing)
            ref_depth, ref_index = VR.reference(N, W, H, s)
            ref_img, ref_err = VR.colour(ref_index, labels, colors)
            assert ref_err == 0
            img, depth, index = V.render_points(x, l, colors, cam, point_size=s, near=VR.NEAR, far=VR.FAR, return_depth=True,
                                                return_index=True)
            assert img.dtype == torch.uint8 and img.shape == (H, W, 3)
            assert depth.dtype == torch.float32 and depth.shape == (H, W) and index.dtype == torch.int32 and index.shape == (H, W)
            assert np.array_equal(index.cpu().numpy(), ref_index), (N, s)
            assert same_bits(depth.cpu().numpy(), ref_depth), (N, s)
            assert np.array_equal(img.cpu().numpy(), ref_img), (N, s)
        if N == 2048:                                      # two runs: byte-identical; a coloured and an image background
            again = V.render_points(x, l, torch.from_numpy(colors).to(dev), cam, point_size=5, near=VR.NEAR, far=VR.FAR)
            assert torch.equal(again, img)
            got = V.render_points(x, l, colors, cam, point_size=5, background=(7, 0, 250), near=VR.NEAR, far=VR.FAR)
            assert np.array_equal(got.cpu().numpy(), VR.colour(ref_index, labels, colors, (7, 0, 250))[0])
            bg = np.random.default_rng(8).integers(0, 256, size=(H, W, 3)).astype(np.uint8)
            bg_dev = torch.from_numpy(bg).to(dev)
            got = V.render_points(x, l, colors, cam, point_size=5, background=bg_dev, near=VR.NEAR, far=VR.FAR)
            assert np.array_equal(got.cpu().numpy(), VR.colour(ref_index, labels, colors, bg)[0])
            assert np.array_equal(bg_dev.cpu().numpy(), bg)                     # the background is read, never written


def test_points_are_read_in_place(dev):
    W, H, N = 53, 37, 2048
    cam, colors = camera_of(VR.unit_camera(W, H)), palette()
    pts = VR.cloud(N, W, H)
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, 19, N).astype(np.int64)).to(dev)
    x = torch.from_numpy(pts.copy()).to(dev)
    rows = torch.cat([x, torch.full((N, 1), float("nan"), device=dev)], 1)     # [N, 4] scan rows, pitch 4
    want = V.render_points(x, labels, colors, cam, 2, near=VR.NEAR, far=VR.FAR, return_depth=True, return_index=True)
    assert np.array_equal(want[2].cpu().numpy(), VR.reference(N, W, H, 2)[1])
    for view in (rows[:, :3], rows):
        got = V.render_points(view, labels, colors, cam, 2, near=VR.NEAR, far=VR.FAR, return_depth=True, return_index=True)
        assert all(same_tensor(a, b) for a, b in zip(got, want))
    assert V._xyz_rows(rows[:, :3], "test")[0].data_ptr() == rows.data_ptr()   # no copy was made


def test_preallocated_buffers_capture_into_a_graph(dev):
    W, H, N, s = 53, 37, 2048, 3
    cam, colors = camera_of(VR.unit_camera(W, H)), torch.from_numpy(palette()).to(dev)
    x = torch.from_numpy(VR.cloud(N, W, H).copy()).to(dev)
    labels = torch.from_numpy(np.random.default_rng(2).integers(0, 19, N).astype(np.int64)).to(dev)
    eager = V.render_points(x, labels, colors, cam, s, near=VR.NEAR, far=VR.FAR, return_depth=True, return_index=True)
    assert np.array_equal(eager[2].cpu().numpy(), VR.reference(N, W, H, s)[1])
    out = torch.full((H, W, 3), 77, device=dev, dtype=torch.uint8)
    zkey = torch.zeros(H * W, device=dev, dtype=torch.int64)                   # stale contents: the call clears it itself
    owner = torch.full((H * W,), -1, device=dev, dtype=torch.int32)
    depth = torch.zeros(H, W, device=dev, dtype=torch.float32)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    run = lambda: V.render_points(x, labels, colors, cam, s, near=VR.NEAR, far=VR.FAR, out=out, zkey=zkey, owner=owner, depth=depth,
                                  err=err)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert run() is out
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(depth.view(torch.int32), eager[1].view(torch.int32))
    assert torch.equal(owner.view(H, W) - 1, eager[2]) and int(err.item()) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        out.zero_()
        depth.zero_()
        owner.zero_()
        zkey.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(depth.view(torch.int32), eager[1].view(torch.int32))
        assert torch.equal(owner.view(H, W) - 1, eager[2]) and int(err.item()) == 0


def kitti_scan():
    n = syn.kitti_cloud(77, 6000, 6000, 1)[:, :4]
    return np.stack([n[:, 0] * 70, n[:, 1] * 70, n[:, 2] * 3, n[:, 3] / 2 + 0.5], 1).astype(np.float32)


def test_the_references_own_camera(dev):
    cam, ref_cam, s = fixture_cameras()
    assert s == 2 and (cam.width, cam.height) == (800, 800)
    scan = kitti_scan()
    labels = np.random.default_rng(9).integers(0, 19, len(scan)).astype(np.int64)
    colors = palette()
    drawn, d, xw, yw, _ = VR.project(scan[:, :3], ref_cam, 0.1, 1000.0)
    x0, y0 = np.array(VR.first_cells(xw, s)), np.array(VR.first_cells(yw, s))
    inside = drawn & (x0 >= 0) & (x0 < 800) & (y0 >= 0) & (y0 < 800)
    assert int(inside.sum()) == 5993                                           # occlusion and ties are plentiful:
    assert len(set(zip(x0[inside].tolist(), y0[inside].tolist()))) == 3596     # ... 5 993 squares start on 3 596 pixels
    assert len(np.unique(d)) == 3770                                           # ... 3 770 float32 depths among 6 000 points
    ref_depth, ref_index = VR.paint(scan[:, :3], ref_cam, s, 0.1, 1000.0)
    ref_img, _ = VR.colour(ref_index, labels, colors)
    rows = torch.from_numpy(scan).to(dev)                                      # [N, 4] rows, read in place; the default planes
    img, depth, index = V.render_points(rows, torch.from_numpy(labels).to(dev), colors, cam, point_size=s, return_depth=True,
                                        return_index=True)
    assert np.array_equal(index.cpu().numpy(), ref_index)
    assert same_bits(depth.cpu().numpy(), ref_depth)
    assert np.array_equal(img.cpu().numpy(), ref_img) and ref_img.any()


def test_frame_segmenter_ego_view(dev):
    from pointnet12_amd.pointnet2 import PointNet2SemSeg
    g = golden("g18_kitti_view.npz")
    cal, colors = V.Calibration(g["R"], g["T"], g["P"]), g["colors"]
    cam, ref_cam, s = fixture_cameras()
    scan = kitti_scan()
    torch.manual_seed(0)
    model = PointNet2SemSeg(19, feature_dims=1).to(dev).eval()
    seg = V.FrameSegmenter(model, cal, colors, npoints=2048, image_size=(375, 1242), camera=cam, point_size=s)
    choice = np.random.default_rng(5).integers(0, len(scan), 2048)
    out = seg.frame(scan, choice=choice)
    pred = out["pred"].cpu().numpy()
    picked = scan[choice]
    # teacher-forced: the restatement draws with the pipeline's own predictions
    _, ref_index = VR.paint(picked[:, :3], ref_cam, s, 0.1, 1000.0)
    ref_img, ref_err = VR.colour(ref_index, pred, colors)
    assert ref_err == 0 and ref_img.any()
    assert out["ego_view"].shape == (800, 800, 3) and out["ego_view"].dtype == torch.uint8
    assert np.array_equal(out["ego_view"].cpu().numpy(), ref_img)
    RT = np.concatenate((g["R"], g["T"]), axis=1)                              # the other two pictures are what they were
    ref_cam_img, _ = KR.draw(KR.pixels(KR.project(picked[:, :3], RT, g["P"])), pred, colors, (375, 1242), V.DISC_HALF_WIDTHS[2])
    assert np.array_equal(out["image"].cpu().numpy(), ref_cam_img)
    assert int(seg.error_flag.item()) == 0
    eager = [out[k].clone() for k in ("ego_view", "image", "top_view")]

    lp, raw, pts = out["log_probs"].clone(), seg.raw_rows.clone(), out["points"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seg.render(lp, raw, pts)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seg.render(lp, raw, pts)
    for _ in range(2):
        seg.ego_view.zero_()
        seg.image.zero_()
        seg.top_view.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((seg.ego_view, seg.image, seg.top_view), eager))
    assert int(seg.error_flag.item()) == 0

    plain = V.FrameSegmenter(model, cal, colors, npoints=2048, image_size=(375, 1242))
    out2 = plain.frame(scan, choice=choice)
    assert "ego_view" not in out2 and not hasattr(plain, "ego_view") and not hasattr(plain, "_zkey")
    assert torch.equal(out2["image"], eager[1]) and torch.equal(out2["top_view"], eager[2])


def test_labels_and_arguments(dev, tmp_path):
    W, H, N = 53, 37, 257
    cam, colors = camera_of(VR.unit_camera(W, H)), palette(5)
    pts = VR.cloud(N, W, H)
    x = torch.from_numpy(pts.copy()).to(dev)
    labels = np.random.default_rng(3).integers(0, 5, N).astype(np.int64)
    ref_index = VR.reference(N, W, H, 2)[1]
    bad = labels.copy()
    bad[np.unique(ref_index[ref_index >= 0])[::2]] = 5                          # every second VISIBLE point has no colour
    ref_bad, ref_err = VR.colour(ref_index, bad, colors, (3, 2, 1))
    assert ref_err == 1 and not np.array_equal(ref_bad, VR.colour(ref_index, labels, colors, (3, 2, 1))[0])
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    got = V.render_points(x, torch.from_numpy(bad).to(dev), colors, cam, 2, background=(3, 2, 1), near=VR.NEAR, far=VR.FAR, err=err)
    assert np.array_equal(got.cpu().numpy(), ref_bad) and int(err.item()) == 1
    with pytest.raises(IndexError):
        V.render_points(x, torch.from_numpy(bad).to(dev), colors, cam, 2, near=VR.NEAR, far=VR.FAR)
    neg = labels.copy()
    neg[:] = -1
    with pytest.raises(IndexError):
        V.render_points(x, torch.from_numpy(neg).to(dev), colors, cam, 2, near=VR.NEAR, far=VR.FAR)
    l = torch.from_numpy(labels).to(dev)
    with pytest.raises(_lib.Pn2Error, match="unsupported"):
        V.render_points(x, l, colors, cam, point_size=17)                        # PN2_EUNSUPPORTED
    for near, far in ((1.0, 1.0), (2.0, 1.0), (0.0, 10.0), (-1.0, 10.0)):
        with pytest.raises(_lib.Pn2Error, match="invalid argument"):
            V.render_points(x, l, colors, cam, near=near, far=far)
    with pytest.raises(ValueError):
        V.render_points(x, l, colors, cam, point_size=2.5)
    with pytest.raises(RuntimeError):
        V.render_points(x.double(), l, colors, cam)
    with pytest.raises(ValueError):
        V.render_points(x, l.int(), colors, cam)
    with pytest.raises(_lib.Pn2Error):
        V.render_points(x.cpu(), l, colors, cam)
    with pytest.raises(ValueError):
        V.render_points(x, l, colors, cam, zkey=torch.empty(H * W, device=dev, dtype=torch.int32))
    # the parsers feed the renderer: files written here from the fixture's numbers draw what the objects built by hand draw
    g = golden("g19_ego_view.npz")
    (tmp_path / "cam.json").write_text(json.dumps({"extrinsic": g["extrinsic"].tolist(), "unknown": 1, "intrinsic": {
        "width": 800, "height": 800, "intrinsic_matrix": g["intrinsic_matrix"].tolist()}}))
    (tmp_path / "opt.json").write_text(json.dumps({"point_size": float(g["point_size"]), "background_color": [0.0, 0.0, 1.0]}))
    cam_file, opt = V.PinholeCamera.from_json(str(tmp_path / "cam.json")), V.RenderOption.from_json(str(tmp_path / "opt.json"))
    cam_hand, ref_cam, _ = fixture_cameras()
    far_pts = torch.from_numpy(np.float32([[10, 0, 0], [10, 1, 0.5], [20, -3, 1]])).to(dev)
    l3 = torch.tensor([0, 1, 2], device=dev)
    a = V.render_points(far_pts, l3, colors, cam_file, opt.point_size, opt.background_color)
    b = V.render_points(far_pts, l3, colors, cam_hand, 2, (0, 0, 255))
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), VR.colour(VR.paint(far_pts.cpu().numpy(), ref_cam, 2, 0.1, 1000.0)[1], [0, 1, 2], colors, (0, 0, 255))[0])
