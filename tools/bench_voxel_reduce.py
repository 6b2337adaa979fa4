#!/usr/bin/env python3
"""Voxel mean and majority label on the HIP library (``pn2_segment_mean`` / ``pn2_segment_mean_bwd`` / ``pn2_segment_mode``, through
``voxel.VoxelGrid`` and ``voxel.segment_mean`` / ``segment_mode``) against stock torch on the same device, in the same run.

    python tools/bench_voxel_reduce.py [--reps 20] [--seed 0] [--only scan,scans16,clouds,onecell]

Prints one JSON line.  The three workloads of tools/bench_voxel.py (scan: 120 000 rows at 0.1 m; scans16: 16 of them in one launch;
clouds: 16 x 4 096 normalised rows at 0.02) and ``onecell``: 120 000 rows that ALL fall into one cell, the contention worst case
(every atomic of a pass lands on one accumulator row).  Per workload, medians of --reps runs after 3 warm-up runs, host clock around
the device work (a synchronize on either side), all candidates alternating inside one loop:

  first_ms          ``downsample(out=...)`` with ``reduce="first"``: the grid alone
  mean_mode_ms      the same call with ``reduce="mean", label_reduce="mode"``: the grid plus both reductions
  mean_ms, mode_ms, bwd_ms        each reduction on its own (``inverse`` / ``count`` / ``n_points`` as the grid left them, preallocated
                    outputs and workspace), the mean over all 4 columns
  mean_plain_ms, mode_plain_ms    the same with option PN2_SEGRED_COMBINE = 0: every row issues its own atomics instead of one per
                    run of equal segments inside the wave (the bytes are the same: ``same_bytes``)
  mean_rowlane_ms   the mean with option PN2_SEGRED_LANES = 0: one row per lane and its columns in a loop, instead of lane L holding
                    column L % C of row L / C (run combining on; the same bytes again)
  torch_mean_ms     stock torch: ``zeros.index_add_(0, segment, rows)`` of the float32 rows, divided by the counts
  torch_mode_ms     stock torch: ``bincount(segment * classes + label)`` viewed ``[segments, classes]``, ``argmax(1)`` (19 classes; a
                    table of segments x classes, which the HIP kernel does not need: it has no class limit)
  torch_mean_moved  how far stock torch's float mean moves between two runs of its own on the same input: elements whose bits differ
                    and the largest difference in units of the last place -- float atomics add in arrival order
  mean_moved        the same for ``pn2_segment_mean`` (0 by construction)
  mean_vs_fp64      the largest |mean - fp64 mean| in units of the float32 last place, ours and torch's
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

from bench_voxel import scanner_scan, timed_ms        # noqa: E402  (the workloads of tools/bench_voxel.py, drawn the same way)
from pointnet12_amd import _lib, synthetic, voxel     # noqa: E402

CLASSES = 19


def moved(a, b):
    """(elements whose bits differ, largest difference in float32 units of the last place) between two float32 tensors."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    key = lambda i: torch.where(i < 0, -(i & 0x7FFFFFFF), i)             # sign-magnitude bits -> a monotone integer
    d = (key(ia) - key(ib)).abs()
    return int((d != 0).sum()), int(d.max()) if d.numel() else 0


def ulps_from(reference64, got):
    """Largest |got - reference| in units of got's float32 last place (1.0 = one ulp)."""
    got64 = got.double()
    spacing = torch.ldexp(torch.ones_like(got64), (torch.frexp(got64.abs().clamp(min=2.0 ** -126))[1] - 24).int())
    return float(((got64 - reference64).abs() / spacing).max()) if got.numel() else 0.0


def workload(name, B, M, size, reps, dev, rng):
    if name == "clouds":
        pts = np.concatenate([synthetic.kitti_cloud(int(rng.integers(1 << 30)), M)[:, :4] for _ in range(B)], 0)
    elif name == "onecell":
        pts = rng.uniform(0.01, 0.09, size=(B * M, 4)).astype(np.float32)
    else:
        pts = np.concatenate([scanner_scan(rng, M) for _ in range(B)], 0)
    points = torch.from_numpy(pts).to(dev)
    labels = torch.from_numpy(rng.integers(0, CLASSES, B * M).astype(np.int32)).to(dev)
    begin = torch.arange(B, device=dev, dtype=torch.int64) * M
    count = torch.full((B,), M, device=dev, dtype=torch.int64)
    first, both = voxel.VoxelGrid(size, device=dev), voxel.VoxelGrid(size, device=dev, reduce="mean", label_reduce="mode")
    bufs_first, bufs = first.buffers(B * M, B, M), both.buffers(B * M, B, M)
    run_first = lambda: first.downsample(points, labels, begin, count, M, out=bufs_first)
    run_both = lambda: both.downsample(points, labels, begin, count, M, out=bufs)
    run_both()
    both.check()
    # the reductions on their own, on what the grid left behind
    inverse, n_points, voxels = bufs.inverse, bufs.n_points, bufs.count
    mean_out = torch.zeros(B * M, 4, device=dev)
    mode_out, votes = torch.zeros(B * M, dtype=torch.int32, device=dev), torch.zeros(B * M, dtype=torch.int32, device=dev)
    grad_in, grad_out = torch.zeros(B * M, 4, device=dev), torch.randn(B * M, 4, device=dev)
    ws, err = bufs.reduce_workspace, torch.zeros(1, dtype=torch.int32, device=dev)
    lib, p = _lib.load(), _lib.ptr
    run_mean = lambda: voxel.segment_mean(points, inverse, voxels, n_points, begin, count, M, out=mean_out, error_flag=err, workspace=ws)
    run_mode = lambda: voxel.segment_mode(labels, inverse, voxels, -1, False, begin, count, M, out=mode_out, votes=votes, error_flag=err,
                                          workspace=ws)
    run_bwd = lambda: _lib.check(lib.pn2_segment_mean_bwd(p(grad_out), 4, 4, p(inverse), p(begin), p(count), B, M, p(begin), p(voxels),
                                                          p(n_points), p(grad_in), 4, p(err), _lib.stream()), "pn2_segment_mean_bwd")

    def with_option(name, fn):
        def run():
            _lib.set_option(name, 0)
            try:
                fn()
            finally:
                _lib.set_option(name, 1)
        return run

    plain = lambda fn: with_option("PN2_SEGRED_COMBINE", fn)

    # stock torch: one global segment number per row (cloud b's segments start at b * M)
    segment = (inverse.long() + torch.arange(B, device=dev).repeat_interleave(M) * M)
    assert int(inverse.min()) >= 0
    pop = torch.bincount(segment, minlength=B * M).clamp(min=1).float().unsqueeze(1)
    torch_mean = lambda: torch.zeros(B * M, 4, device=dev).index_add_(0, segment, points) / pop
    pair = segment * CLASSES + labels.long()
    torch_mode = lambda: torch.bincount(pair, minlength=B * M * CLASSES).view(B * M, CLASSES).argmax(1)

    runs = {"first_ms": run_first, "mean_mode_ms": run_both, "mean_ms": run_mean, "mode_ms": run_mode, "bwd_ms": run_bwd,
            "mean_plain_ms": plain(run_mean), "mode_plain_ms": plain(run_mode), "mean_rowlane_ms": with_option("PN2_SEGRED_LANES", run_mean),
            "torch_mean_ms": torch_mean, "torch_mode_ms": torch_mode}
    for fn in runs.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in runs}
    for _ in range(reps):                                 # alternating: all share whatever else the machine does
        for k, fn in runs.items():
            times[k].append(timed_ms(fn))
    res = {"B": B, "rows": M, "voxel": size, "voxels": int(voxels.sum())}
    res.update({k: round(float(np.median(v)), 4) for k, v in times.items()})
    # what was computed: the same bytes with and without the run combining, and from run to run; torch's own drift
    run_mean()
    run_mode()
    ours, ours_mode = mean_out.clone(), mode_out.clone()
    plain(run_mean)()
    plain(run_mode)()
    res["same_bytes"] = bool(torch.equal(ours.view(torch.int32), mean_out.view(torch.int32)) and torch.equal(ours_mode, mode_out))
    with_option("PN2_SEGRED_LANES", run_mean)()
    res["same_bytes"] = bool(res["same_bytes"] and torch.equal(ours.view(torch.int32), mean_out.view(torch.int32)))
    run_mean()
    res["mean_moved"] = list(moved(ours, mean_out))
    t1, t2 = torch_mean(), torch_mean()
    res["torch_mean_moved"] = list(moved(t1, t2))
    used = torch.cat([torch.arange(int(v), device=dev) + b * M for b, v in enumerate(voxels.cpu().tolist())])
    exact = (torch.zeros(B * M, 4, device=dev, dtype=torch.float64).index_add_(0, segment, points.double()) / pop.double())[used]
    res["mean_vs_fp64"] = {"hip_ulp": round(ulps_from(exact, ours[used]), 3), "torch_ulp": round(ulps_from(exact, t1[used]), 3)}
    res["same_mode"] = bool(torch.equal(ours_mode[used].long(), torch_mode()[used]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="scan,scans16,clouds,onecell")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_voxel_reduce.py needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"scan": (1, 120000, 0.1), "scans16": (16, 120000, 0.1), "clouds": (16, 4096, 0.02), "onecell": (1, 120000, 0.1)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = workload(name, *shapes[name], args.reps, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
