#!/usr/bin/env python3
"""The criterion of the SemanticKITTI loop, forward + backward: loss.cross_entropy (pn2_cross_entropy_fwd / _bwd) against stock
``F.cross_entropy`` on the same device in the same run, on the reference's criterion shapes.

    python tools/bench_loss.py [--reps 20] [--shapes 16x19x8000t,16x19x50000t,65536x13,32768x50]

A shape ``BxCxNt`` is the transposed view of a contiguous [B, N, C] tensor of log-probabilities (pcdseg.py:178-179: KITTI
``inview`` at N = 8000, ``all`` at N = 50000), ``BxCxN`` a contiguous [B, C, N] tensor, ``RxC`` a contiguous [R, C] matrix
(65536x13: S3DIS, 32768x50: ShapeNet parts).  Prints one JSON line; per shape, in microseconds, medians of --reps runs after
warm-up, the two implementations taken in turn inside every repetition:
  eager_us, stock_eager_us    loss + backward to the input, launched from Python (event-timed)
  replay_us, stock_replay_us  the same captured by graph.GraphedStep and replayed (event-timed per replay)
  value_rel_diff_to_stock     |ours - stock| / |stock| of the loss value
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                          # noqa: E402
import torch.nn.functional as F                       # noqa: E402

from pointnet12_amd import graph                      # noqa: E402
from pointnet12_amd.loss import cross_entropy         # noqa: E402


def median_us(fns, reps, warmup=3):
    """Median device time (events) of each callable, the callables taken in turn inside every repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            e.synchronize()
            t.append(a.elapsed_time(e) * 1e3)
    return [float(np.median(t)) for t in times]


def make_input(spec, dev, gen):
    dims = spec.rstrip("t").split("x")
    if len(dims) == 2:
        R, C = int(dims[0]), int(dims[1])
        base = torch.log_softmax(torch.randn(R, C, generator=gen) * 3, -1).to(dev)
        return base, (lambda t: t), torch.randint(0, C, (R,), generator=gen).to(dev)
    B, C, N = (int(v) for v in dims)
    tgt = torch.randint(0, C, (B, N), generator=gen).to(dev)
    if spec.endswith("t"):
        base = torch.log_softmax(torch.randn(B, N, C, generator=gen) * 3, -1).to(dev)
        return base, (lambda t: t.transpose(2, 1)), tgt
    return (torch.randn(B, C, N, generator=gen) * 3).to(dev), (lambda t: t), tgt


def bench_shape(spec, reps, dev):
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

    eager = [step(cross_entropy, leaves[0]), step(F.cross_entropy, leaves[1])]
    t_eager = median_us(eager, reps)
    with torch.no_grad():
        a, b = float(cross_entropy(view(base), tgt)), float(F.cross_entropy(view(base), tgt))
    graphs = [graph.GraphedStep(fn, dev).graph for fn in eager]          # captured as the training step is (graph.py)
    t_replay = median_us([g.replay for g in graphs], reps)
    return {"eager_us": round(t_eager[0], 1), "stock_eager_us": round(t_eager[1], 1), "replay_us": round(t_replay[0], 1),
            "stock_replay_us": round(t_replay[1], 1), "value_rel_diff_to_stock": abs(a - b) / abs(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="16x19x8000t,16x19x50000t,65536x13,32768x50")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "cross_entropy_fwd_bwd", "device": torch.cuda.get_device_name(0), "reps": args.reps, "shapes": {}}
    for s in args.shapes.split(","):
        res["shapes"][s] = bench_shape(s, args.reps, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
