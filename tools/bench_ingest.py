#!/usr/bin/env python3
"""Scan ingest on the HIP library (``kitti.ScanFilter``, ``pn2_scan_filter``) against the host body of ``kitti.read_scan`` (the
numpy restatement of ``Semantic_KITTI_Utils.get``: class map, class drop, view filter, boolean indexing), in the same run.

    python tools/bench_ingest.py [--rows 120000] [--batch 16] [--reps 20] [--seed 0]

Prints one JSON line.  The scans are synthetic (seeded, SemanticKITTI's raw classes through the learning map recorded in
tests/golden/g9_kitti.npz); file reading is excluded on both sides.  Three workloads:

  inview   one scan of --rows rows, subset 'inview'
  all      one scan of --rows rows, subset 'all'
  batch    --batch such scans back to back, subset 'inview', one batched launch

  host_ms      the host way: the numpy body of read_scan on arrays already in memory (per scan; the batch is a loop); median of --reps
  upload_ms    the host-to-device copy of the raw rows and label words (pageable memory), which the device way needs first
  eager_ms     ScanFilter.filter into preallocated buffers, host clock to the end of the device work
  graph_ms     the same call captured in a graph, replayed
  kernel_us    the three launches of pn2_scan_filter together (device events around the eager call)
  kept         rows kept by the device / by the host (they differ only by points within a few float32 steps of a border)

Every figure is a median of --reps runs after 3 warm-up runs.
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

from pointnet12_amd import kitti                      # noqa: E402


def synthetic_scan(rng, rows, raw_classes):
    pts = rng.normal(size=(rows, 4)) * np.array([40.0, 40.0, 3.0, 0.0]) + np.array([8.0, 0.0, -1.0, 0.0])
    pts[:, 3] = rng.random(rows)
    words = raw_classes[rng.integers(0, len(raw_classes), rows)].astype(np.uint32) | (rng.integers(0, 1 << 16, rows).astype(np.uint32) << np.uint32(16))
    return pts.astype(np.float32), words.astype(np.uint32)


def host_body(points, raw, lut, subset):
    """kitti.read_scan without the two np.fromfile calls."""
    sem = raw & 0xFFFF
    label = lut[sem]
    if (label < 0).any():
        raise KeyError(int(sem[label < 0][0]))
    label = label.astype(np.int32)
    keep = label != 0
    points, label = points[keep], label[keep] - 1
    if subset == "inview":
        m = kitti.in_view(points)
        points, label = points[m], label[m]
    return points, label


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


def workload(scans, lmap, lut64, subset, reps, dev):
    B = len(scans)
    counts = np.array([len(p) for p, _ in scans], np.int64)
    raw_h = np.ascontiguousarray(np.concatenate([p for p, _ in scans], 0))
    words_h = np.ascontiguousarray(np.concatenate([w for _, w in scans], 0))
    res = {"scans": B, "rows": int(counts.sum()), "subset": subset}
    host_out = {}

    def host():
        host_out["kept"] = sum(len(host_body(p, w, lut64, subset)[0]) for p, w in scans)
    res["host_ms"] = median_ms(host, reps, sync=False)

    up = {}

    def upload():
        up["raw"] = torch.from_numpy(raw_h).to(dev)
        up["words"] = torch.from_numpy(words_h.view(np.int32)).to(dev)
    res["upload_ms"] = median_ms(upload, reps)
    sf = kitti.ScanFilter(lmap, subset, device=dev)
    begin = torch.from_numpy(np.cumsum(counts) - counts).to(dev)
    count = torch.from_numpy(counts).to(dev)
    max_rows = int(counts.max())
    bufs = sf.buffers(len(raw_h), B, max_rows)
    call = lambda: sf.filter(up["raw"], up["words"], begin, count, max_rows, out=bufs)
    res["eager_ms"] = median_ms(call, reps)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernel = []
    for _ in range(reps):
        torch.cuda.synchronize()
        start.record()
        call()
        end.record()
        torch.cuda.synchronize()
        kernel.append(start.elapsed_time(end) * 1e3)
    res["kernel_us"] = round(float(np.median(kernel)), 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    res["graph_ms"] = median_ms(graph.replay, reps)
    res["kept"] = [int(bufs.count.sum().item()), int(host_out["kept"])]
    res["error_flag"] = int(sf.error_flag.item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "g9_kitti.npz"), allow_pickle=False)
    lmap = {int(k): int(v) for k, v in zip(g["map_keys"], g["map_values"])}
    lut64 = np.full(max(lmap) + 1, -1, np.int64)
    for k, v in lmap.items():
        lut64[k] = v
    raw_classes = np.array(sorted(lmap))
    rng = np.random.default_rng(args.seed)
    dev = torch.device("cuda:0")
    scans = [synthetic_scan(rng, args.rows, raw_classes) for _ in range(args.batch)]
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "inview": workload(scans[:1], lmap, lut64, "inview", args.reps, dev),
           "all": workload(scans[:1], lmap, lut64, "all", args.reps, dev),
           "batch": workload(scans, lmap, lut64, "inview", args.reps, dev)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
