#!/usr/bin/env python3
"""One frame of the reference's KITTI demo (``python pcdvis.py``) on the HIP library: scan -> labels -> pixels -> two images,
three with ``--ego``.

    python tools/demo_kitti.py [--out DIR] [--npoints 25000] [--seed 0] [--merge] [--time] [--raw [--labels-out FILE [--instances SIZE [--boxes-out FILE]]]] [--normals K[:RADIUS]] [--ground THRESHOLD]] [--ego CAMERA.json [--render-option FILE.json]] [--image FILE]
    python tools/demo_kitti.py --root $KITTI_ROOT --part 01 --index 0 --calib DIR --config semantic-kitti.yaml [--checkpoint CKPT]

Without ``--root`` the scan is synthetic (``synthetic.kitti_cloud``, un-normalised back to metres), the calibration is the one
recorded in tests/golden/g18_kitti_view.npz and the network (the zoo's ``PointNet2SemSeg(19, feature_dims=1)``) has seeded random
weights, so the colours mean nothing; the point is the path.  With ``--root`` the scan, its camera image, the calibration files
(``--calib``: the directory holding calib_velo_to_cam.txt and calib_cam_to_cam.txt) and the dataset's yaml (``--config``) are read
from disk, and ``--checkpoint`` loads reference weights.  ``FrameSegmenter`` does the rest on the device; the two images are
written as PNG through PIL (``semantic.png``: the camera view, ``top_view.png``).  Neither cv2 nor open3d is used.

``--ego CAMERA.json`` (an open3d ``PinholeCameraParameters`` file, the reference's ``config/ego_view.json``) adds the demo's 3-D ego
view (``Window_Manager.update``, pcdvis.py:31-51) as ``ego_view.png``; ``--render-option FILE.json`` (an open3d ``RenderOption``
file, the reference's ``config/render_option.json``) sets its point size and background colour (defaults: 2, black).  The picture follows the rule stated in include/pn2.h, which is unverified against open3d.

``--image FILE`` (any picture PIL reads; ``synthetic``: ``synthetic.camera_image``) is the camera frame for the image -> points
direction: every drawn row takes the colour of the pixel under it (``FrameSegmenter.frame(image=)``, ``pn2_sample_image``; no depth
test, as in the reference) and ``painted.png`` shows those rows drawn with THEIR OWN camera colour on black
(``draw_2d_points(labels=None, colors=[N, 3])``): the coloured cloud as the camera sees it.  With ``--root`` the frame read from the
dataset stays the background of ``semantic.png``; FILE must have its size.

``--raw`` feeds the RAW scan through ``FrameSegmenter.frame_raw``: the class map, the class drop, the view filter and the
compaction run on the device (``kitti.ScanFilter``, ``pn2_scan_filter``) and the kept count never leaves it; the synthetic scan has
no label file (a live feed), a dataset scan goes in with its ``.label`` words.  The choice is then drawn on the device.
``--labels-out FILE`` (with ``--raw``, without ``--merge``) goes through ``FrameSegmenter.label_scan`` instead: every row of the
raw scan takes the majority label of its 5 nearest drawn rows within 1 m, mapped back to the dataset's raw ids
(``kitti.inverse_label_lut``), rows the filter dropped are 0, and FILE is written in the dataset's ``.label`` format.
``--instances SIZE`` (with ``--labels-out``) fills the words' HIGH halves too: the kept rows' predicted classes are gridded at SIZE
metres and the cells of the "thing" classes (training classes 0 .. 7: car .. motorcyclist) are clustered per class under 26
connectivity (``kitti_view.InstanceSpec``, ``voxel.VoxelGrid.components``, ``pn2_voxel_components``); a row's instance is ``id + 1``, 0
for none, and the low halves are what they are without the option, byte for byte.
``--boxes-out FILE`` (with ``--instances``) writes one text line per instance, ``x y z l w h yaw class n``: the oriented box of
``boxes.instance_boxes`` (``pn2_segment_boxes``; metres and radians, the longer side first, yaw in [0, pi)), the instance's majority
training class and its rows.
``--voxel SIZE`` (with ``--raw``) downsamples the kept rows to one row per occupied cell of SIZE metres before the choice
(``voxel.VoxelGrid``, ``pn2_voxel_grid``), which is then drawn from the voxel count.  ``--voxel-reduce mean`` shows each cell's mean row
(centroid and mean remission, ``pn2_segment_mean``) instead of its first, ``--voxel-labels mode`` takes the cell's majority label.

``--search grid`` runs the neighbour search of ``--labels-out`` and ``--normals`` on the uniform grid of ``neighbors.GridIndex`` instead of
by ``pn2_knn``'s brute force (``--normals`` then needs its RADIUS); the default, ``brute``, leaves both as they were.

``--normals K[:RADIUS]`` (with ``--raw``) writes one more picture, ``normals.png``: the surface normal of every drawn row from its K
nearest drawn rows (within RADIUS metres, if given), turned towards the scanner (``normals.estimate_normals(viewpoint="origin")``,
``pn2_knn`` + ``pn2_local_pca``), as the camera view with colour ``round(127.5 * (n + 1))`` per component
(``draw_2d_points(labels=None, colors=)``); a row with fewer than three neighbours in reach has a zero normal and is mid-grey.
Without the option the tool's output is what it is without it, byte for byte.

``--ground THRESHOLD`` (with ``--raw``) writes one more picture, ``ground.png``: the drawn rows within THRESHOLD metres of the scan's
ground plane -- ``plane.ground_labels(threshold=THRESHOLD, max_angle=15)``: RANSAC with the normal held within 15 degrees of +z, two
least-squares refits (``pn2_plane_ransac`` / ``pn2_plane_refit`` / ``pn2_plane_classify``) -- in brown, the rest in green, as the camera
view (``draw_2d_points(labels=None, colors=)``), and prints the plane.  No network is involved.  Without the option every output of
the tool is what it is without it, byte for byte.

``--time`` prints one JSON line with medians of 20 (device work included, host clock) for the post-network stages --
predict + project + both images (``render_ms``), and the same as a captured graph (``render_graph_ms``) -- and beside them, in
the same run, the same stages the way the reference goes about them, written in this project's own words: an arg-max read back
to the host (``ref_argmax_ms``), an fp32 stock-torch projection of a host array with its upload and read-back
(``ref_project_ms``), and -- only if ``cv2`` imports, else null -- one filled ``cv2.circle`` per point on the host
(``ref_draw_ms``: a median of 3, not of 20; the loop takes tens of milliseconds).  With ``--ego`` also the ego view's stage alone
(``ego_ms``: depth test, resolve and colouring into the segmenter's buffers) beside a stock-torch z-buffer of the same picture
(``ref_zbuffer_ms``: fp64 projection, packed int64 (depth bits, index) keys, ``scatter_reduce(..., "amin")`` per square offset,
colours gathered from the winners); ``ego_matches_ref`` says whether the two pictures are equal.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                          # noqa: E402

from pointnet12_amd import kitti_view as V            # noqa: E402
from pointnet12_amd import synthetic as syn           # noqa: E402
from pointnet12_amd.pointnet2 import PointNet2SemSeg, load_reference_state   # noqa: E402

# the merge list of the reference's SemKITTI_2_Common comes from the caller; this is the demo's own choice of merges
MERGE = ["road", "parking+sidewalk+other-ground", "building+fence", "vegetation+trunk+terrain", "pole+traffic-sign",
         "person+bicyclist+motorcyclist", "car+truck+other-vehicle", "motorcycle+bicycle"]


def synthetic_inputs(seed):
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_kitti_view.npz"), allow_pickle=False)
    n = syn.kitti_cloud(seed, 60000, 60000, 1)[:, :4]
    scan = np.stack([n[:, 0] * 70, n[:, 1] * 70, n[:, 2] * 3, n[:, 3] / 2 + 0.5], 1).astype(np.float32)
    cfg = {k: dict(zip(g[k + "_keys"].tolist(), g[k + "_values"].tolist())) for k in ("labels", "color_map", "learning_map_inv")}
    return scan, None, V.Calibration(g["R"], g["T"], g["P"]), cfg, None


def dataset_inputs(args):
    import yaml
    from PIL import Image
    from pointnet12_amd import kitti
    cfg = yaml.safe_load(open(args.config))
    seq = os.path.join(args.root, "sequences", args.part)
    words = None
    if args.raw:
        scan = np.fromfile(os.path.join(seq, "velodyne", "%06d.bin" % args.index), dtype=np.float32).reshape(-1, 4)
        words = np.fromfile(os.path.join(seq, "labels", "%06d.label" % args.index), dtype=np.uint32)
    else:
        scan, _ = kitti.read_scan(os.path.join(seq, "velodyne", "%06d.bin" % args.index), os.path.join(seq, "labels", "%06d.label" % args.index),
                                  cfg["learning_map"], "inview")
    fn = os.path.join(seq, "image_2", "%06d.png" % args.index)
    frame = np.asarray(Image.open(fn).convert("RGB")) if os.path.exists(fn) else None
    calib = V.Calibration.from_files(os.path.join(args.calib, "calib_velo_to_cam.txt"), os.path.join(args.calib, "calib_cam_to_cam.txt"))
    return scan, frame, calib, cfg, words


def host_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4)


def baseline_project(points_host, calib, dev):
    """The projection as a stock-torch user would write it around a host array: upload, fp32 rotation + translation, fp32
    camera matrix, perspective division, read back -- the shape of work (two host round trips, fp32 products) that the
    reference's torch formulation does, in this project's own words."""
    rot = torch.as_tensor(calib.R, dtype=torch.float32, device=dev)
    shift = torch.as_tensor(calib.T.reshape(3), dtype=torch.float32, device=dev)
    cam = torch.as_tensor(calib.P, dtype=torch.float32, device=dev)
    homog = (torch.as_tensor(points_host, device=dev) @ rot.T + shift) @ cam.T
    return (homog[:, :2] / homog[:, 2:3]).cpu().numpy()


def baseline_zbuffer(pts, labels, colors, cam, s, background=(0, 0, 0), near=0.1, far=1000.0):
    """The ego view as a stock-torch user would write it: fp64 pinhole projection, one int64 key per point (float32 depth bits
    above the index), a ``scatter_reduce`` minimum per offset of the square, then colours gathered from the winning indices."""
    dev = pts.device
    H, W = cam.height, cam.width
    E = torch.as_tensor(cam.E, device=dev)
    fx, fy, cx, cy = cam.K.tolist()
    c = pts[:, :3].double() @ E[:, :3].T + E[:, 3]
    Z = c[:, 2]
    xw, yw = fx * c[:, 0] / Z + cx + 0.5, fy * c[:, 1] / Z + cy + 0.5
    ok = (Z > near) & (Z < far) & (xw.abs() < 2.0 ** 30) & (yw.abs() < 2.0 ** 30)
    half = 0.5 if s % 2 == 0 else 0.0
    x0 = torch.floor(torch.where(ok, xw, torch.zeros_like(xw)) + half).long() - s // 2
    y0 = torch.floor(torch.where(ok, yw, torch.zeros_like(yw)) + half).long() - s // 2
    key = (Z.float().view(torch.int32).long() << 32) | torch.arange(len(pts), device=dev)
    empty = torch.iinfo(torch.int64).max
    zbuf = torch.full((H * W,), empty, device=dev, dtype=torch.int64)
    for dy in range(s):
        for dx in range(s):
            x, y = x0 + dx, y0 + dy
            m = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            zbuf.scatter_reduce_(0, (y * W + x)[m], key[m], "amin")
    seen = zbuf != empty
    img = torch.as_tensor(background, device=dev, dtype=torch.uint8).expand(H * W, 3).contiguous()
    img[seen] = colors[labels[(zbuf[seen] & 0xffffffff)]]
    return img.view(H, W, 3)


def timings(seg, out, calib, colors, frame):
    lp, raw, pts = out["log_probs"].clone(), seg.raw_rows.clone(), out["points"].clone()
    bg = None if frame is None else torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    res = {"npoints": seg.npoints, "image": list(seg.image_size), "device": torch.cuda.get_device_name(0)}
    res["render_ms"] = host_ms(lambda: seg.render(lp, raw, pts, bg))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seg.render(lp, raw, pts, bg)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seg.render(lp, raw, pts, bg)
    res["render_graph_ms"] = host_ms(graph.replay)
    pred = {}

    def ref_argmax():
        pred["v"] = lp.argmax(-1).cpu().numpy()
    res["ref_argmax_ms"] = host_ms(ref_argmax)
    points_host = raw[:, :3].cpu().numpy()
    pixels = {}

    def ref_project():
        pixels["v"] = baseline_project(points_host, calib, raw.device)
    res["ref_project_ms"] = host_ms(ref_project)
    if seg.camera is not None:
        cam, s = seg.camera, seg.point_size
        option_background = (0, 0, 0) if isinstance(seg._ego_background, tuple) else seg._ego_background[0, 0].tolist()
        owner = seg._owner[:cam.height * cam.width]
        res["ego"] = [cam.height, cam.width, s]
        res["ego_ms"] = host_ms(lambda: V.render_points(raw, seg.pred, seg.colors, cam, s, out=seg.ego_view, zkey=seg._zkey, owner=owner,
                                                        background=seg._ego_background, err=seg.error_flag))
        picture = {}

        def ref_zbuffer():
            picture["v"] = baseline_zbuffer(raw, seg.pred, seg.colors, cam, s, option_background)
        res["ref_zbuffer_ms"] = host_ms(ref_zbuffer)
        res["ego_matches_ref"] = bool(torch.equal(picture["v"], seg.ego_view))
    res["ref_draw_ms"] = None
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None and seg.groups is None:
        H, W = seg.image_size
        canvas = np.zeros((H, W, 3), np.uint8) if frame is None else np.ascontiguousarray(frame)
        centres = [tuple(c) for c in np.nan_to_num(pixels["v"], nan=-1e6, posinf=-1e6, neginf=-1e6).clip(-1e6, 1e6).astype(np.int32).tolist()]
        paint = [tuple(int(v) for v in colors[k]) for k in pred["v"]]

        def ref_draw():                                    # one filled circle per point on the host, in point order
            picture = canvas.copy()
            for k in range(len(centres)):
                cv2.circle(picture, centres[k], seg.radius, paint[k], -1)
        res["ref_draw_ms"] = host_ms(ref_draw, reps=3, warmup=1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="demo_out")
    ap.add_argument("--npoints", type=int, default=25000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--merge", action="store_true", help="predict over the demo's merged classes")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--raw", action="store_true", help="feed the raw scan through frame_raw: filter and compaction on the device")
    ap.add_argument("--labels-out", metavar="FILE", help="with --raw: label every row of the scan (label_scan) and write a .label file")
    ap.add_argument("--instances", type=float, metavar="SIZE",
                    help="with --labels-out: Euclidean clustering of the thing classes on a grid of SIZE metres; instance ids in the high halves")
    ap.add_argument("--normals", metavar="K[:RADIUS]", help="with --raw: also write normals.png, the drawn rows' surface normals as colours")
    ap.add_argument("--ground", type=float, metavar="THRESHOLD", help="with --raw: also write ground.png, the drawn rows on / off the RANSAC ground plane")
    ap.add_argument("--boxes-out", metavar="FILE", help="with --instances: one line per instance, x y z l w h yaw class n (boxes.instance_boxes)")
    ap.add_argument("--search", choices=("brute", "grid"), default="brute",
                    help="the neighbour search of --labels-out and --normals: pn2_knn's brute force, or the uniform grid of neighbors.GridIndex "
                         "(--normals then needs a RADIUS)")
    ap.add_argument("--voxel", type=float, metavar="SIZE", help="with --raw: voxel-grid downsample the kept rows at SIZE metres")
    ap.add_argument("--voxel-reduce", choices=("first", "mean"), default="first",
                    help="with --voxel: a cell is shown by its first row or by the mean of its rows")
    ap.add_argument("--voxel-labels", choices=("first", "mode"), default="first",
                    help="with --voxel: a cell's label is its first row's or the majority of its rows'")
    ap.add_argument("--ego", metavar="CAMERA.json", help="also draw the 3-D ego view through this open3d PinholeCameraParameters file")
    ap.add_argument("--render-option", metavar="FILE.json", help="open3d RenderOption file: the ego view's point size and background colour")
    ap.add_argument("--image", metavar="FILE", help="camera frame to colour the drawn rows from ('synthetic': a generated one); writes painted.png")
    ap.add_argument("--root")
    ap.add_argument("--part", default="01")
    ap.add_argument("--index", type=int, default=0)
    ap.add_argument("--calib")
    ap.add_argument("--config")
    ap.add_argument("--checkpoint")
    args = ap.parse_args()
    from PIL import Image

    if args.root:
        if not (args.calib and args.config):
            ap.error("--root needs --calib and --config")
        scan, frame, calib, cfg, words = dataset_inputs(args)
    else:
        scan, frame, calib, cfg, words = synthetic_inputs(args.seed)
    names, colors, _ = V.classes_from_config(cfg)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    model = PointNet2SemSeg(len(names), feature_dims=1)
    if args.checkpoint:
        state = torch.load(args.checkpoint, map_location="cpu")
        load_reference_state(model, state.get("model_state_dict", state) if isinstance(state, dict) else state)
    model = model.cuda().eval()
    groups = V.merge_groups(names, MERGE, colors) if args.merge else None
    size = (375, 1242) if frame is None else frame.shape[:2]
    camera_image = None
    if args.image:
        camera_image = syn.camera_image(args.seed, *size) if args.image == "synthetic" else \
            np.ascontiguousarray(np.asarray(Image.open(args.image).convert("RGB")))
        if frame is None:
            size = camera_image.shape[:2]
        elif camera_image.shape[:2] != tuple(size):
            ap.error("--image must have the dataset frame's size, %d x %d" % tuple(size))
        camera_image = torch.from_numpy(camera_image).cuda()
    if args.render_option and not args.ego:
        ap.error("--render-option needs --ego")
    if args.labels_out and (not args.raw or args.merge):
        ap.error("--labels-out needs --raw and does not go with --merge (merged classes have no raw id)")
    if args.instances is not None and not args.labels_out:
        ap.error("--instances needs --labels-out")
    if args.boxes_out and args.instances is None:
        ap.error("--boxes-out needs --instances")
    if args.voxel is None and (args.voxel_reduce != "first" or args.voxel_labels != "first"):
        ap.error("--voxel-reduce / --voxel-labels need --voxel")
    if args.voxel is not None and not args.raw:
        ap.error("--voxel needs --raw")
    if args.normals and not args.raw:
        ap.error("--normals needs --raw")
    if args.ground is not None and not args.raw:
        ap.error("--ground needs --raw")
    camera = V.PinholeCamera.from_json(args.ego) if args.ego else None
    option = V.RenderOption.from_json(args.render_option) if args.render_option else V.RenderOption()
    seg = V.FrameSegmenter(model, calib, colors if groups is None else groups.colors, npoints=args.npoints, image_size=size, groups=groups,
                           camera=camera, point_size=option.point_size, ego_background=option.background_color, color_mode="rgb",
                           color_normalize=False)
    if args.raw:
        from pointnet12_amd import kitti
        scan_filter = kitti.ScanFilter(cfg["learning_map"] if words is not None else None, "inview")
        gen = torch.Generator(device="cuda")
        gen.manual_seed(args.seed)
        grid = None
        if args.voxel is not None:
            from pointnet12_amd import voxel
            grid = voxel.VoxelGrid(args.voxel, reduce=args.voxel_reduce, label_reduce=args.voxel_labels)
        if args.labels_out:
            out = seg.label_scan(scan, words, scan_filter=scan_filter, rng=gen, lut=kitti.inverse_label_lut(cfg["learning_map_inv"]),
                                 background=frame, voxel=grid, image=camera_image, search=args.search,
                                 instances=None if args.instances is None else V.InstanceSpec(args.instances, range(8),
                                                                                                boxes=bool(args.boxes_out)))
            kitti.write_labels(args.labels_out, out["scan_labels"], out.get("scan_instances"))
            print("labelled %d of %d rows; wrote %s" % (int((out["scan_labels"] != 0).sum()), len(scan), args.labels_out))
            if args.instances is not None:
                print("%d instances of the thing classes on %d rows (cells of %g m)"
                      % (int(out["instance_count"].item()), int((out["scan_instances"] != 0).sum()), args.instances))
            if args.boxes_out:
                from pointnet12_amd import boxes, voxel as VX
                S = int(out["instance_count"].item())
                b = boxes.canonical(out["instance_boxes"])
                classes = VX.segment_mode(out["kept_classes"], out["kept_instances"], out["instance_count"], row_begin=seg._raw_state["begin"],
                                          row_count=out["count"])
                table = torch.cat([b.center[:S], b.size[:S], b.yaw[:S, None]], 1).cpu().numpy()
                with open(args.boxes_out, "w") as f:
                    for row, c, n in zip(table, classes[:S].cpu().tolist(), b.n[:S].cpu().tolist()):
                        f.write("%.3f %.3f %.3f %.3f %.3f %.3f %.4f %d %d\n" % (*row, c, n))
                print("wrote %d boxes to %s" % (S, args.boxes_out))
        else:
            out = seg.frame_raw(scan, words, scan_filter=scan_filter, rng=gen, background=frame, voxel=grid, image=camera_image)
        print("raw scan of %d rows, %d kept by the device filter; filter error flag %d"
              % (len(scan), int(out["count"].item()), int(scan_filter.error_flag.item())))
        if grid is not None:
            print("%d voxels of %g m; grid error flag %d" % (int(out["voxel_count"].item()), args.voxel, int(grid.error_flag.item())))
    else:
        out = seg.frame(scan, background=frame, image=camera_image)
    os.makedirs(args.out, exist_ok=True)
    Image.fromarray(out["image"].cpu().numpy()).save(os.path.join(args.out, "semantic.png"))
    Image.fromarray(out["top_view"].cpu().numpy()).save(os.path.join(args.out, "top_view.png"))
    if camera is not None:
        Image.fromarray(out["ego_view"].cpu().numpy()).save(os.path.join(args.out, "ego_view.png"))
        print("ego view %d x %d, point size %d, background %s; wrote %s/ego_view.png"
              % (camera.height, camera.width, option.point_size, option.background_color, args.out))
    if camera_image is not None:
        valid = out["point_valid"]
        pix = torch.where(valid[:, None], out["pix"], torch.full_like(out["pix"], V.INT32_MIN))      # rows outside the frame are not drawn
        painted = V.draw_2d_points(pix, None, out["point_colors"].to(torch.uint8), None, size)
        Image.fromarray(painted.cpu().numpy()).save(os.path.join(args.out, "painted.png"))
        print("%d of %d drawn rows inside the camera frame; wrote %s/painted.png" % (int(valid.sum()), args.npoints, args.out))
    if args.normals:
        from pointnet12_amd import normals as PN
        k, _, radius = args.normals.partition(":")
        n = PN.estimate_normals(seg.raw_rows, k=int(k), radius=float(radius) if radius else None, viewpoint="origin", search=args.search)
        shade = torch.round(127.5 * (n + 1.0)).clamp(0, 255).to(torch.uint8)
        picture = V.draw_2d_points(out["pix"], None, shade, None, size)
        Image.fromarray(picture.cpu().numpy()).save(os.path.join(args.out, "normals.png"))
        print("normals of %d drawn rows from %s neighbours%s, %d of them zero (fewer than three in reach); wrote %s/normals.png"
              % (len(n), k, " within %s m" % radius if radius else "", int((n == 0).all(1).sum()), args.out))
    if args.ground is not None:
        from pointnet12_amd import plane as PL
        buf = PL.buffers(len(seg.raw_rows), 1, 256, device=seg.raw_rows.device)
        ground = PL.ground_labels(seg.raw_rows, threshold=args.ground, max_angle=15.0, buffers=buf) < 0
        shade = torch.where(ground[:, None], torch.tensor([150, 100, 50], device=ground.device), torch.tensor([40, 200, 90], device=ground.device))
        picture = V.draw_2d_points(out["pix"], None, shade.to(torch.uint8), None, size)
        Image.fromarray(picture.cpu().numpy()).save(os.path.join(args.out, "ground.png"))
        print("ground plane n = (%.4f, %.4f, %.4f), d = %.4f m, rmse %.4f m: %d of %d drawn rows within %g m of it; status %d; wrote %s/ground.png"
              % (*buf.plane[0].cpu().tolist(), float(buf.rmse[0]), int(ground.sum()), len(ground), args.ground, int(buf.status[0]), args.out))
    counts = torch.bincount(out["pred"], minlength=len(colors)).cpu().tolist()
    drawn = int((out["pix"][:, 0] != V.INT32_MIN).sum())
    print("scan of %d points resampled to %d; %d with a pixel, %d classes predicted; error flag %d; wrote %s/semantic.png and top_view.png"
          % (len(scan), args.npoints, drawn, sum(c > 0 for c in counts), int(seg.error_flag.item()), args.out))
    if args.time:
        print(json.dumps(timings(seg, out, calib, colors if groups is None else groups.colors, frame)))


if __name__ == "__main__":
    main()
