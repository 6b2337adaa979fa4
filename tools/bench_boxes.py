#!/usr/bin/env python3
"""Segment boxes on the HIP library (``pn2_segment_boxes`` through ``boxes.segment_boxes``) against the same sweep in stock torch on
the same device, in the same run.

    python tools/bench_boxes.py [--reps 20] [--seed 0] [--angles 64] [--split 0] [--only scan,scan_ground,scans16,one]

Prints one JSON line.  Workloads: ``scan``: the one-scan workload of tools/bench_cluster.py (120 000 rows of a scanner model gridded
at 0.1 m), clustered with the ground LEFT IN (the ground is one huge instance: the workgroup sweep's case); ``scan_ground``: the same
scan with ``plane.ground_labels`` taken out first; ``scans16``: 16 such scans in one call (ground left in); each of these with
``min_points`` 1 and 10; ``one``: 120 000 rows in ONE segment, the worst case for the workgroup sweep.  The clustering is done once and
not timed.  Per workload:

  eager_ms   ``segment_boxes(buffers=...)``: every output
  graph_ms   the same call captured into a graph, replayed
  torch_ms   the same sweep in stock torch: ``[N, A]`` projections, ``scatter_reduce`` amin / amax by segment, the score by
             ``index_add_``, the selection by three reductions.  float32 like the kernel's, but torch fuses nothing and orders sums as
             it likes: ``same_angle`` is the share of segments on which both sides name the same angle
  segments, rows_in_segments, largest

Medians of --reps runs after 3 warm-up runs, the two sides alternating, host clock around the device work (a synchronize on either
side).  ``--split`` is ``split_rows`` (0: the library's 4096).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch                                          # noqa: E402

from bench_voxel import scanner_scan, timed_ms        # noqa: E402
from pointnet12_amd import boxes, plane, voxel        # noqa: E402


def torch_sweep(points, seg, S, table, d0):
    """The rule in stock torch for ONE cloud: (angle int64 [S], n)."""
    keep = seg >= 0
    xy, ids = points[keep, :2], seg[keep].long()
    c, s = table[:, 0][None], table[:, 1][None]
    x, y = xy[:, 0:1], xy[:, 1:2]
    u, v = c * x + s * y, c * y - s * x                               # [N, A]
    A = table.shape[0]
    idx = ids[:, None].expand(-1, A)
    full = lambda value: torch.full((S, A), value, device=points.device, dtype=torch.float32)
    u0, u1 = full(float("inf")).scatter_reduce_(0, idx, u, "amin"), full(-float("inf")).scatter_reduce_(0, idx, u, "amax")
    v0, v1 = full(float("inf")).scatter_reduce_(0, idx, v, "amin"), full(-float("inf")).scatter_reduce_(0, idx, v, "amax")
    e = torch.minimum(torch.minimum(u - u0[ids], u1[ids] - u), torch.minimum(v - v0[ids], v1[ids] - v))
    t = (d0 / torch.clamp(e, min=d0) * 1048576.0).to(torch.int64)
    score = torch.zeros(S, A, device=points.device, dtype=torch.int64).index_add_(0, ids, t)
    area = (u1 - u0) * (v1 - v0)
    best = score.max(1, keepdim=True).values
    area = torch.where(score == best, area, torch.full_like(area, float("inf")))
    return area.argmin(1), torch.bincount(ids, minlength=S)


def run(points, seg, count, begin, rows, M, B, angles, d0, split, reps, dev):
    buf = boxes.buffers(B * M, B, M, angles, dev)
    eager = lambda: boxes.segment_boxes(points, seg, count, angles=angles, d0=d0, row_begin=begin, row_count=rows, max_rows=M, buffers=buf,
                                        split_rows=split)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    counts = count.cpu().tolist()
    stock = lambda: [torch_sweep(points[b * M:(b + 1) * M], seg[b * M:(b + 1) * M], max(counts[b], 1), buf.table, d0) for b in range(B)]
    fns = {"eager_ms": eager, "graph_ms": graph.replay, "torch_ms": stock}
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed_ms(fn))
    res = {k: round(float(np.median(v)), 4) for k, v in times.items()}
    eager()
    torch.cuda.synchronize()
    same, total, largest, inside = 0, 0, 0, 0
    for b, (angle, n) in enumerate(stock()):
        mine = buf.angle[b * M:b * M + counts[b]].long()
        same += int((mine == angle[:counts[b]]).sum().item())
        total += counts[b]
        if counts[b]:
            largest, inside = max(largest, int(buf.n[b * M:b * M + counts[b]].max().item())), inside + int(buf.n[b * M:b * M + counts[b]].sum().item())
    res.update({"segments": total, "rows_in_segments": inside, "largest": largest, "same_angle": round(same / max(total, 1), 4),
                "error_flag": int(buf.error_flag.item())})
    return res


def workload(name, args, dev, rng):
    B, M = (16, 120000) if name == "scans16" else (1, 120000)
    pts = np.concatenate([scanner_scan(rng, M) for _ in range(B)], 0)
    points = torch.from_numpy(pts).to(dev)
    begin = torch.arange(B, device=dev, dtype=torch.int64) * M
    rows = torch.full((B,), M, device=dev, dtype=torch.int64)
    res = {"B": B, "rows": M}
    if name == "one":
        seg = torch.zeros(M, device=dev, dtype=torch.int32)
        res["one"] = run(points, seg, torch.ones(1, device=dev, dtype=torch.int64), begin, rows, M, B, args.angles, args.d0, args.split, args.reps, dev)
        return res
    labels = None
    if name == "scan_ground":
        labels = plane.ground_labels(points[:, :3].contiguous(), threshold=0.2, max_angle=15.0)
        res["ground_rows"] = int((labels < 0).sum().item())
    vg = voxel.VoxelGrid(0.1, device=dev, label_reduce="mode")
    down = vg.downsample(points, labels, begin, rows, M, out=vg.buffers(B * M, B, M))
    for min_points in (1, 10):
        comps = vg.components(points, down, row_labels=labels, min_points=min_points, row_begin=begin, row_count=rows, max_rows=M,
                              out=vg.component_buffers(B * M, B, M))
        vg.check()
        res["min_points_%d" % min_points] = run(points, comps.row_component, comps.count, begin, rows, M, B, args.angles, args.d0, args.split,
                                                args.reps, dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--angles", type=int, default=64)
    ap.add_argument("--d0", type=float, default=0.05)
    ap.add_argument("--split", type=int, default=0)
    ap.add_argument("--only", default="scan,scan_ground,scans16,one")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_boxes.py needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    out = {"reps": args.reps, "angles": args.angles, "d0": args.d0, "split_rows": args.split, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = workload(name, args, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
