#!/usr/bin/env python3
"""Voxel-grid downsampling on the HIP library (``pn2_voxel_grid`` through ``voxel.VoxelGrid.downsample``) against stock torch on
the same device, in the same run.

    python tools/bench_voxel.py [--reps 20] [--seed 0] [--only scan,scans16,clouds]

Prints one JSON line.  Three workloads, synthetic and seeded:

  scan     one scan of 120 000 rows at 0.1 m: a 64-beam scanner model in metres (ground rings and obstacles out to 70 m, 2 cm of
           noise), so rows crowd near the sensor as a real scan's do
  scans16  16 such scans back to back in one launch
  clouds   16 x 4 096 normalised rows at 0.02: ``synthetic.kitti_cloud``, the training batch's distribution, drawn WITH replacement
           (duplicate rows included)

  eager_ms  ``downsample(out=...)`` into preallocated buffers: every output (points, labels, index, count, inverse, n_points)
  graph_ms  the same call captured into a graph, replayed
  stock_ms  the stock formulation: the three cells in fp64, packed into one int64 key per row (the cloud number above them),
            ``torch.unique(return_inverse=True, return_counts=True)``, ``scatter_reduce(amin)`` of the row numbers for the
            representatives and a gather of their rows (16 bits per axis suffice for these workloads).  It sorts, synchronises
            with the host for the output size and returns the voxels in KEY order, not in the scan's; it is timed as it is
  voxels    the number of voxels, which must be the same on both sides (``same_voxels``: also the same representatives)

Every time is a median of --reps runs after 3 warm-up runs, host clock around the device work (a synchronize on either side); the
two sides alternate inside one loop.
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

from pointnet12_amd import synthetic, voxel           # noqa: E402


def scanner_scan(rng, rows):
    """One revolution of a 64-beam scanner in metres: float32 ``[rows, 4]`` (the model of ``synthetic.kitti_cloud``, all round)."""
    phi = np.deg2rad(np.linspace(-24.8, 2.0, 64))[rng.integers(0, 64, size=rows)]
    theta = np.deg2rad(rng.uniform(-180.0, 180.0, size=rows))
    with np.errstate(divide="ignore"):
        rho_ground = np.where(phi < np.deg2rad(-1.0), 1.73 / np.tan(-phi), np.inf)
    rho = np.minimum(np.minimum(rho_ground, 5.0 + rng.exponential(20.0, size=rows)), 70.0)
    xyz = np.stack([rho * np.cos(phi) * np.cos(theta), rho * np.cos(phi) * np.sin(theta), rho * np.sin(phi)], 1)
    xyz = xyz + rng.normal(0.0, 0.02, size=xyz.shape)
    return np.concatenate([xyz, rng.uniform(0.0, 1.0, size=(rows, 1))], 1).astype(np.float32)


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stock(points, labels, size, B, M):
    """Stock torch on ``[B * M, ld]``: (points, labels, index, count per cloud, inverse, n_points), voxels in key order."""
    q = torch.floor(points[:, :3].double() / size).long() + (1 << 15)      # (the workloads' cells fit 16 bits an axis)
    cloud = torch.arange(B, device=points.device).repeat_interleave(M)
    key = (cloud << 48) | (q[:, 0] << 32) | (q[:, 1] << 16) | q[:, 2]
    uniq, inverse, n_points = torch.unique(key, return_inverse=True, return_counts=True)
    row = torch.arange(points.shape[0], device=points.device)
    first = torch.full((uniq.shape[0],), points.shape[0], device=points.device, dtype=torch.int64)
    first = first.scatter_reduce(0, inverse, row, "amin")
    count = torch.bincount(uniq >> 48, minlength=B)
    return points[first], labels[first], first, count, inverse, n_points


def workload(name, B, M, size, reps, dev, rng):
    if name == "clouds":
        pts = np.concatenate([synthetic.kitti_cloud(int(rng.integers(1 << 30)), M)[:, :4] for _ in range(B)], 0)
    else:
        pts = np.concatenate([scanner_scan(rng, M) for _ in range(B)], 0)
    points = torch.from_numpy(pts).to(dev)
    labels = torch.from_numpy(rng.integers(0, 19, B * M).astype(np.int32)).to(dev)
    begin = torch.arange(B, device=dev, dtype=torch.int64) * M
    count = torch.full((B,), M, device=dev, dtype=torch.int64)
    vg = voxel.VoxelGrid(size, device=dev)
    bufs = vg.buffers(B * M, B, M)
    eager = lambda: vg.downsample(points, labels, begin, count, M, out=bufs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    runs = {"eager_ms": eager, "graph_ms": graph.replay, "stock_ms": lambda: stock(points, labels, size, B, M)}
    for fn in runs.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in runs}
    for _ in range(reps):                                 # alternating: the three share whatever else the machine does
        for k, fn in runs.items():
            times[k].append(timed_ms(fn))
    res = {"B": B, "rows": M, "voxel": size}
    res.update({k: round(float(np.median(v)), 4) for k, v in times.items()})
    eager()
    vg.check()
    s_pts, s_lab, s_first, s_count, _, s_pop = stock(points, labels, size, B, M)
    mine = bufs.count.cpu()
    res["voxels"] = int(mine.sum())
    same = torch.equal(mine, s_count.cpu())
    if same:                                              # the same representatives and populations, brought into one order
        reps_mine = torch.cat([bufs.index[b * M:b * M + int(mine[b])].long() + b * M for b in range(B)])
        pop_mine = torch.cat([bufs.n_points[b * M:b * M + int(mine[b])].long() for b in range(B)])
        order = torch.argsort(s_first)
        same = torch.equal(reps_mine, s_first[order]) and torch.equal(pop_mine, s_pop[order])
    res["same_voxels"] = bool(same)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="scan,scans16,clouds")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_voxel.py needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"scan": (1, 120000, 0.1), "scans16": (16, 120000, 0.1), "clouds": (16, 4096, 0.02)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = workload(name, *shapes[name], args.reps, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
