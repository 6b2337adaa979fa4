#!/usr/bin/env python3
"""The camera colour lookup on the HIP library (``pn2_project_points`` + ``pn2_sample_image``: ``kitti_view.paint_points``) against
two baselines in the same run.

    python tools/bench_image.py [--reps 20] [--seed 0] [--points 120000] [--scans 16] [--only single,batch]

Prints one JSON line.  Two workloads, synthetic and seeded (``synthetic.kitti_scan`` in metres, ``synthetic.camera_image`` frames of
375 x 1242, the calibration recorded in tests/golden/g18_kitti_view.npz), mode HSV, normalised: the reference's stored target.

  single   120 000 points into one frame
  batch    16 scans of 120 000 points, each into its own frame, in ONE project launch and ONE sample launch

  paint_ms       project + sample into preallocated [M, 7] rows (two launches, nothing read back)
  sample_ms      pn2_sample_image alone, on the pixels already projected
  stock_ms       stock torch on the device: an fp32 projection (matmuls and a division), the truncation, the in-image mask and
                 advanced indexing into a PRECOMPUTED float HSV frame, then the two divisions -- the frame's conversion is not
                 timed (the reference converts at load time too), for the batch a flat [B * H * W, 3] frame indexed with the
                 cloud number
  host_loop_ms   `single` only: the reference's own way (data_utils/ColorGenerator_Loader.py:59-69) on the host -- numpy projection, then
                 the per-point Python loop over the 120 000 pixels into the precomputed HSV frame, then the divisions (one run takes
                 about a tenth of a second)
  equal_stock    fraction of rows on which stock torch and the library agree bit for bit.  They need not: the stock projection is
                 fp32 where the library follows numpy's fp64 products, and how stock torch divides by a host scalar on the device
                 is its own matter
  equal_host     `single`: whether the host loop and the library agree bit for bit on every row (they state the same rule)

Every device time is a median of --reps runs after 3 warm-up runs, host clock around the device work (a synchronize on either side).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                          # noqa: E402

import image_sample_ref as R                          # noqa: E402
from pointnet12_amd import kitti_view as V            # noqa: E402
from pointnet12_amd import synthetic as syn           # noqa: E402

H, W = 375, 1242


def median_ms(fn, reps, warmup=3, sync=True):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4)


def stock_paint(rows, RT, P, frame_flat, cloud, out):
    """Stock torch ops: fp32 projection, truncation, mask, advanced indexing into the flat float HSV frame(s), the divisions."""
    xyz1 = torch.cat([rows[:, :3], torch.ones_like(rows[:, :1])], 1)
    q = (xyz1 @ RT.T) @ P.T
    uv = (q[:, :2] / q[:, 2:3]).to(torch.int32).long()
    x, y = uv[:, 0], uv[:, 1]
    ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    flat = (cloud * H + y.clamp(0, H - 1)) * W + x.clamp(0, W - 1)
    c = frame_flat[flat] * ok[:, None]
    c[:, 0] /= 180
    c[:, 1:] /= 255
    out[:, :4] = rows
    out[:, 4:] = c
    return out


def host_loop(scan, calib, frame_hsv):
    """The reference's way on the host (ColorGenerator_Loader.py:59-69, restated): the numpy projection, one Python iteration per point
    into the precomputed HSV frame, the divisions over the finished array."""
    ones = np.ones((len(scan), 1), np.float32)
    cam = (calib.RT @ np.hstack([scan[:, :3], ones]).T).astype(np.float32)
    img = (calib.P @ cam).astype(np.float32)
    with np.errstate(all="ignore"):
        pixels = (img[:2] / img[2]).T.astype(np.int32)
    rows, cols = frame_hsv.shape[:2]
    colors = np.zeros((len(scan), 3), np.float32)
    for n, (col, row) in enumerate(pixels):
        if 0 <= row < rows and 0 <= col < cols:
            colors[n] = frame_hsv[row, col]
    colors[:, 0] /= 180
    colors[:, 1:] /= 255
    return np.hstack([scan, colors])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--only", default="single,batch")
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_kitti_view.npz"), allow_pickle=False)
    calib = V.Calibration(g["R"], g["T"], g["P"])
    RT, P = torch.from_numpy(calib.RT).float().to(dev), torch.from_numpy(calib.P).float().to(dev)
    res = {"tool": "bench_image", "reps": args.reps, "points": args.points, "image": [H, W], "mode": "hsv"}
    for name in args.only.split(","):
        B = 1 if name == "single" else args.scans
        M = B * args.points
        scans = [syn.kitti_scan(args.seed + b, args.points) for b in range(B)]
        images = np.stack([syn.camera_image(args.seed + b, H, W) for b in range(B)])
        frames = np.stack([R.color_frame(im, "hsv", "rgb") for im in images])
        rows = torch.from_numpy(np.concatenate(scans)).to(dev)
        image = torch.from_numpy(images).to(dev)
        frame_flat = torch.from_numpy(frames).to(dev).view(-1, 3)
        cloud = torch.arange(B, device=dev).repeat_interleave(args.points)
        count = torch.full((B,), args.points, device=dev, dtype=torch.int64)
        begin = torch.arange(B, device=dev, dtype=torch.int64) * args.points
        out = torch.empty(M, 7, device=dev)
        pix = torch.empty(M, 2, device=dev, dtype=torch.int32)
        valid = torch.empty(M, device=dev, dtype=torch.uint8)
        stock_out = torch.empty(M, 7, device=dev)

        def paint():
            V.paint_points(rows, calib, image, "hsv", True, "rgb", out=out, pix=pix, valid=valid, row_begin=begin, row_count=count,
                           max_rows=args.points)

        def sample():
            V.sample_image(pix, image, "hsv", True, "rgb", out[:, 4:], valid, begin, count, args.points)

        r = {"clouds": B, "paint_ms": median_ms(paint, args.reps), "sample_ms": median_ms(sample, args.reps),
             "stock_ms": median_ms(lambda: stock_paint(rows, RT, P, frame_flat, cloud, stock_out), args.reps)}
        same = (out.view(torch.int32) == stock_out.view(torch.int32)).all(1)
        r["equal_stock"] = round(float(same.float().mean()), 6)
        r["valid_fraction"] = round(float(valid.float().mean()), 4)
        if name == "single":
            host = {}
            r["host_loop_ms"] = median_ms(lambda: host.update(v=host_loop(scans[0], calib, frames[0])), args.reps, warmup=1, sync=False)
            r["equal_host"] = bool(host["v"].tobytes() == out.cpu().numpy().tobytes())
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
