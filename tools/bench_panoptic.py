#!/usr/bin/env python3
"""Panoptic counts on the HIP library (``metrics.panoptic_counts`` -> ``pn2_panoptic_count``) against the host formulation of the same
rule (tests/panoptic_ref.py: numpy, one ``np.unique`` per class and side, as the SemanticKITTI API's evaluator works), in the same run.

    python tools/bench_panoptic.py [--reps 20] [--seed 0] [--only scan,scans16,onesegment]

Prints one JSON line.  Workloads: ``scan``: one 120 000-row scan with a realistic segment mix (tools/eval_panoptic.py,
``synthetic_pair``: a few stuff segments of tens of thousands of rows, 120 things, rows in runs); ``scans16``: 16 such scans in one
call; ``onesegment``: 120 000 rows that are ALL one segment on both sides, the contention worst case (every area and intersection
atomic of the count launch lands on one word unless the wave combines them first).  Per workload, medians of --reps runs after 3
warm-up runs, host clock around the device work (a synchronize on either side), the device candidates alternating inside one loop:

  eager_ms   ``panoptic_counts(..., out=, work=)``: four launches, nothing allocated, nothing read back
  graph_ms   the same call captured once and replayed
  host_ms    ``panoptic_ref.panoptic_table`` on numpy arrays that are already on the host (no transfer counted; median of
             ``host_reps`` runs)
  same       the device table equals the host table, int64 for int64
The library's wave combining is a compile-time constant (``make XFLAGS=-DPN2_PANOPTIC_COMBINE=0`` builds the uncombined form); the
line reports which build ran as far as the caller knows (``--label``).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                          # noqa: E402

import panoptic_ref                                   # noqa: E402
from eval_panoptic import CLASSES, THINGS, class_masks, synthetic_pair      # noqa: E402
from pointnet12_amd import metrics                    # noqa: E402


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def workload(name, B, M, reps, host_reps, dev, seed):
    include, things = class_masks(CLASSES, THINGS)
    if name == "onesegment":
        host = [np.full(B * M, v, np.int32) for v in (9, 0, 9, 0)]
    else:
        scans = [synthetic_pair(seed + b, M) for b in range(B)]
        host = [np.concatenate([s[k] for s in scans]) for k in range(4)]
    d = [torch.from_numpy(a).to(dev) for a in host]
    begin = torch.arange(B, device=dev, dtype=torch.int64) * M
    count = torch.full((B,), M, device=dev, dtype=torch.int64)
    inc_d, th_d = torch.from_numpy(include).to(dev), torch.from_numpy(things).to(dev)
    out = torch.zeros(CLASSES, 5, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    work = metrics.panoptic_workspace(B, M, dev)
    run = lambda: metrics.panoptic_counts(d[0], d[1], d[2], d[3], CLASSES, inc_d, th_d, 30, begin, count, M, out=out, err=err, work=work)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    begins, counts = [b * M for b in range(B)], [M] * B
    on_host = lambda: panoptic_ref.panoptic_table(host[0], host[1], host[2], host[3], CLASSES, include, things, 30, begins, counts)
    runs = {"eager_ms": run, "graph_ms": graph.replay}
    for fn in runs.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in list(runs) + ["host_ms"]}
    for _ in range(reps):                                 # alternating: all share whatever else the machine does
        for k, fn in runs.items():
            times[k].append(timed_ms(fn))
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = on_host()[0]
        times["host_ms"].append((time.perf_counter() - t0) * 1e3)
    out.zero_()
    run()
    got = out.cpu().numpy()
    res = {"B": B, "rows": M, "host_reps": host_reps, "matches": int(got[:, 0].sum()), "fp": int(got[:, 1].sum()), "fn": int(got[:, 2].sum())}
    res.update({k: round(float(np.median(v)), 4) for k, v in times.items()})
    res["same"] = bool(np.array_equal(got, want)) and int(err.item()) == 0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="scan,scans16,onesegment")
    ap.add_argument("--host-reps", type=int, default=None, help="runs of the host formulation per workload (default: --reps, a third of it "
                    "for the 16-scan workload, whose host pass takes seconds)")
    ap.add_argument("--label", default="combine=1", help="which build of the library this is (free text, copied into the line)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_panoptic.py needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda")
    shapes = {"scan": (1, 120000), "scans16": (16, 120000), "onesegment": (1, 120000)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "build": args.label}
    for name in args.only.split(","):
        host_reps = args.host_reps if args.host_reps is not None else max(1, args.reps // (3 if shapes[name][0] > 1 else 1))
        out[name] = workload(name, *shapes[name], args.reps, host_reps, dev, args.seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
