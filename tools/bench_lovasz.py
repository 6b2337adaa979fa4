#!/usr/bin/env python3
"""The Lovasz-Softmax loss, forward + backward: loss.lovasz_softmax (pn2_lovasz_fwd / _bwd, one segmented radix sort for all classes)
against the authors' formulation written in stock torch -- softmax, then per class one ``torch.sort``, a gather and two ``cumsum``s in
a Python loop, classes="present" -- on the same device in the same run, on bench_loss.py's four shapes.

    python tools/bench_lovasz.py [--reps 20] [--shapes 16x19x8000t,16x19x50000t,65536x13,32768x50] [--ours-only]

No row is ignored, so that the stock side can be timed at all (it compacts ignored rows by boolean indexing).  THE STOCK FORMULATION
CANNOT BE CAPTURED INTO A GRAPH: ``if fg.sum() == 0`` reads a count back to the host once per class; it is timed eagerly in both
columns.  Prints one JSON line; per shape, in microseconds, medians of --reps runs after warm-up on the host clock with the device
work included (a synchronize closes every timed call), the implementations taken in turn inside every repetition:
  eager_us         ours, loss + backward to the input, launched from Python
  replay_us        ours, captured by graph.GraphedStep and replayed
  stock_eager_us   the stock formulation, eager (the only way it runs)
  value_rel_diff_to_stock   |ours - stock| / |stock| of the loss value
``--ours-only`` runs nothing of the stock side (for a kernel trace of the launches of ours alone).
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
import torch.nn.functional as F                       # noqa: E402

from pointnet12_amd import graph                      # noqa: E402
from pointnet12_amd.loss import lovasz_softmax        # noqa: E402
from bench_loss import make_input                     # noqa: E402


def stock_lovasz_softmax(x, target):
    """The authors' lovasz_softmax(probas, labels, classes='present') with the softmax in front, as training loops call it."""
    C = x.shape[1]
    probas = F.softmax(x, 1).movedim(1, -1).reshape(-1, C)
    labels = target.reshape(-1)
    losses = []
    for c in range(C):
        fg = (labels == c).float()
        if fg.sum() == 0:                             # a read-back per class
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        gt = fg[perm]
        gts = gt.sum()
        jaccard = 1.0 - (gts - gt.cumsum(0)) / (gts + (1.0 - gt).cumsum(0))
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        losses.append(torch.dot(errors_sorted, jaccard))
    return sum(losses) / len(losses)


def median_host_us(fns, reps, warmup=3):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e6)
    return [float(np.median(t)) for t in times]


def bench_shape(spec, reps, dev, ours_only):
    gen = torch.Generator().manual_seed(len(spec))
    base, view, tgt = make_input(spec, dev, gen)
    leaves = [base.clone().requires_grad_(True) for _ in range(2)]

    def step(f, leaf):
        def run():
            leaf.grad = None
            loss = f(view(leaf), tgt)
            loss.backward()
            return loss
        return run

    ours, stock = step(lovasz_softmax, leaves[0]), step(stock_lovasz_softmax, leaves[1])
    g = graph.GraphedStep(ours, dev).graph
    if ours_only:
        t = median_host_us([ours, g.replay], reps)
        return {"eager_us": round(t[0], 1), "replay_us": round(t[1], 1)}
    t = median_host_us([ours, g.replay, stock], reps)
    with torch.no_grad():
        a, b = float(lovasz_softmax(view(base), tgt)), float(stock_lovasz_softmax(view(base), tgt))
    return {"eager_us": round(t[0], 1), "replay_us": round(t[1], 1), "stock_eager_us": round(t[2], 1),
            "value_rel_diff_to_stock": abs(a - b) / abs(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="16x19x8000t,16x19x50000t,65536x13,32768x50")
    ap.add_argument("--ours-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "lovasz_softmax_fwd_bwd", "device": torch.cuda.get_device_name(0), "reps": args.reps, "shapes": {}}
    for s in args.shapes.split(","):
        res["shapes"][s] = bench_shape(s, args.reps, dev, args.ours_only)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
