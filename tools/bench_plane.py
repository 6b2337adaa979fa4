#!/usr/bin/env python3
"""Plane RANSAC on the HIP library (``pointnet12_amd.plane``) against the same rule in stock torch on the same device, in the same run,
and what removing the ground does to Euclidean clustering.

    python tools/bench_plane.py [--reps 20] [--seed 0] [--only scan,scan1024,scans16,clouds]

Prints one JSON line.  ``scan``: 120 000 rows of a scanner model with 256 hypotheses, ``scan1024``: the same with 1 024, ``scans16``: 16
scans in one call with 256, ``clouds``: 16 x 4 096 normalised rows with 256.  The search is for the ground (``axis = +z``, 15
degrees, threshold 0.1 m; 0.02 on the normalised clouds).  Per workload, sides alternating, medians of --reps runs after 3 warm-up runs,
host clock around the device work (a synchronize on either side):

  ransac_ms   ``pn2_plane_ransac`` alone into preallocated buffers: hypotheses, the all-pairs scoring pass, the select
  stock_ms    the same step in stock torch: three random rows per hypothesis, the planes, the flip and the angle test, then a
              ``[N, 3] @ [3, H]`` fp64 product plus d, a compare and a sum over the rows, an argmax.  It draws its rows with torch's
              generator, so it scores other hypotheses than the library: it is the same WORK, not the same bytes
  fit_ms      ``plane.fit_plane(buffers=)``: ransac, two refit rounds, the classification of every row (9 launches, two fills)
  graph_ms    the same call captured into a graph, replayed
  inliers     the share of the rows within the threshold of the fitted plane (cloud 0)

and, on ``scan`` only, tools/bench_cluster.py's one-scan workload at 0.1 m and connectivity 26 with and without the ground:

  labels_ms            ``plane.ground_labels(buffers=)``
  cluster_ms           ``downsample`` + ``components`` of all rows (labels all 0): the ground is one large component
  cluster_noground_ms  the same with ``ground_labels``' labels: the ground's voxels take no part
  components / components_noground
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch                                          # noqa: E402

from bench_voxel import scanner_scan, timed_ms        # noqa: E402
from pointnet12_amd import _lib, plane, synthetic, voxel   # noqa: E402

COS15 = math.cos(math.radians(15.0))


def stock_ransac(pts, H, threshold, gen):
    """[B,N,ld] float32 -> (plane [B,4] fp64, count [B]): the rule's steps in stock torch, hypotheses drawn by torch's generator."""
    B, N, _ = pts.shape
    p = pts[:, :, :3].double()
    rows = torch.randint(0, N, (B, H, 3), device=pts.device, generator=gen)
    tri = torch.gather(p, 1, rows.reshape(B, H * 3, 1).expand(-1, -1, 3)).reshape(B, H, 3, 3)
    c = torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
    n = c / c.norm(dim=-1, keepdim=True)
    n = torch.where(n[..., 2:] < 0, -n, n)
    valid = n[..., 2] >= COS15                                     # (NaN from a degenerate triple fails)
    d = -(n * tri[:, :, 0]).sum(-1)
    r = torch.baddbmm(d[:, None, :], p, n.transpose(1, 2))         # [B,N,3] @ [B,3,H] + d
    counts = (r.abs() <= threshold).sum(1)
    counts = torch.where(valid, counts, torch.full_like(counts, -1))
    best = counts.argmax(1)
    at = best[:, None, None]
    return torch.cat([n.gather(1, at.expand(-1, -1, 3))[:, 0], d.gather(1, best[:, None])], 1), counts.gather(1, best[:, None])[:, 0]


def alternate(runs, reps):
    for fn in runs.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed_ms(fn))
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def workload(name, B, M, H, threshold, reps, dev, rng):
    if name == "clouds":
        pts = np.stack([synthetic.kitti_cloud(int(rng.integers(1 << 30)), M)[:, :4] for _ in range(B)], 0)
    else:
        pts = np.stack([scanner_scan(rng, M) for _ in range(B)], 0)
    points = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
    buf = plane.buffers(M, B, H, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    lib, p = _lib.load(), _lib.ptr
    axis = plane._axis((0, 0, 1))

    def ransac():
        _lib.check(lib.pn2_plane_ransac(p(points), points.shape[2], B, M, None, None, H, 0, ctypes.addressof(axis), COS15, threshold, p(buf.plane),
                                        None, p(buf.best_h), p(buf.best_count), p(buf.status), p(buf.error_flag), p(buf.workspace),
                                        _lib.stream()), "pn2_plane_ransac")

    fit = lambda: plane.fit_plane(points, threshold, iterations=H, max_angle=15.0, buffers=buf)
    graph = captured(fit)
    res = {"B": B, "rows": M, "iterations": H, "threshold": threshold}
    res.update(alternate({"ransac_ms": ransac, "stock_ms": lambda: stock_ransac(points, H, threshold, gen), "fit_ms": fit,
                          "graph_ms": graph.replay}, reps))
    out = fit()
    buf.check()
    res["inliers"] = round(float(out.count[0].item()) / M, 4)
    res["stock_inliers"] = round(float(stock_ransac(points, H, threshold, gen)[1][0].item()) / M, 4)
    if name == "scan":
        flat = points[0].contiguous()
        vg = voxel.VoxelGrid(0.1, device=dev, label_reduce="mode")
        vbuf, cbuf = vg.buffers(M, 1, M), vg.component_buffers(M, 1, M)
        begin, count = torch.zeros(1, device=dev, dtype=torch.int64), torch.full((1,), M, device=dev, dtype=torch.int64)
        zeros = torch.zeros(M, device=dev, dtype=torch.int32)
        labels = plane.ground_labels(flat, threshold=threshold, max_angle=15.0, iterations=H, buffers=buf).clone()

        def cluster(lab):
            down = vg.downsample(flat, lab, begin, count, M, out=vbuf)
            return vg.components(flat, down, row_labels=lab, connectivity=26, row_begin=begin, row_count=count, max_rows=M, out=cbuf)

        res.update(alternate({"labels_ms": lambda: plane.ground_labels(flat, threshold=threshold, max_angle=15.0, iterations=H, buffers=buf),
                              "cluster_ms": lambda: cluster(zeros), "cluster_noground_ms": lambda: cluster(labels)}, reps))
        res["components"] = int(cluster(zeros).count.sum().item())
        res["components_noground"] = int(cluster(labels).count.sum().item())
        res["ground_rows"] = int((labels < 0).sum().item())
        vg.check()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="scan,scan1024,scans16,clouds")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_plane.py needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"scan": (1, 120000, 256, 0.1), "scan1024": (1, 120000, 1024, 0.1), "scans16": (16, 120000, 256, 0.1), "clouds": (16, 4096, 256, 0.02)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = workload(name, *shapes[name], args.reps, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
