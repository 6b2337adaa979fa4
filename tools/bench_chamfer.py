#!/usr/bin/env python3
"""Chamfer distance on the HIP library (pointnet12_amd/chamfer.py) against stock PyTorch fp32 in the formulation it replaces
(broadcast difference -> norm -> min -> sum, tests/chamfer_ref.py:stock_chamfer), on one GPU.

    python tools/bench_chamfer.py [--reps 20] [--shapes 16x4096x4096,16x4096x1024,1x65536x8192,8x65536x65536]

Prints one JSON line; per shape BxNxM (D = 3):
  fwd_ms, fwdbwd_ms              HIP: chamfer_batch alone / with backward to both inputs (median of --reps event-timed runs after warm-up)
  stock_fwd_ms, stock_fwdbwd_ms  the same for stock torch, same process, runs interleaved with the HIP ones; null where its
                                 [B,N,M,3] intermediates (several of them live at once) would not fit the card's free memory
  search_us                      the nearest-neighbour launches alone (nearest_neighbor: no sum, no backward)
  gpairs_per_s                   B*N*M / search time
  vector_peak_fraction           8 flop per pair (3 subtractions, 1 product, 2 fma) x pairs / search time over the fp32 vector
                                 peak of 157.3 TFLOP/s.  The search is bound by VALU issue, not by bytes (12 B*(N+M) bytes in all).
                                 Note that only the two fma count double in that peak: the loop issues 7 vector instructions per
                                 pair and query (3 + 1 + 2 + compare, plus two selects), packed two queries wide for the first six.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                          # noqa: E402

from pointnet12_amd import chamfer as M               # noqa: E402
import chamfer_ref as C                               # noqa: E402

VECTOR_PEAK_FLOPS = 157.3e12
FLOP_PER_PAIR = 8.0


def median_ms(fns, reps, warmup=3):
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
            t.append(a.elapsed_time(e))
    return [float(np.median(t)) for t in times]


def bench_shape(B, N, Mc, reps, dev):
    gen = torch.Generator(device="cpu").manual_seed(B + N + Mc)
    p1 = (torch.rand(B, N, 3, generator=gen) * 2 - 1).to(dev).requires_grad_(True)
    p2 = (torch.rand(B, Mc, 3, generator=gen) * 2 - 1).to(dev).requires_grad_(True)

    def fwd(f):
        def run():
            with torch.no_grad():
                f(p1, p2)
        return run

    def fwdbwd(f):
        def run():
            p1.grad = p2.grad = None
            f(p1, p2).backward()
        return run

    pairs = float(B) * N * Mc
    free, _ = torch.cuda.mem_get_info(dev)
    stock_fits = pairs * 3 * 4 * 5 < free                # the difference, its square / norm chain and their gradients
    fns = [fwd(M.chamfer_batch), fwdbwd(M.chamfer_batch), lambda: M.nearest_neighbor(p1, p2)]
    if stock_fits:
        fns += [fwd(C.stock_chamfer), fwdbwd(C.stock_chamfer)]
    if pairs > 1e10:
        reps = max(3, reps // 4)
    t = median_ms(fns, reps)
    out = {"fwd_ms": round(t[0], 4), "fwdbwd_ms": round(t[1], 4), "search_us": round(t[2] * 1e3, 1),
           "stock_fwd_ms": round(t[3], 3) if stock_fits else None, "stock_fwdbwd_ms": round(t[4], 3) if stock_fits else None,
           "gpairs_per_s": round(pairs / (t[2] * 1e-3) / 1e9, 1),
           "vector_peak_fraction": round(FLOP_PER_PAIR * pairs / (t[2] * 1e-3) / VECTOR_PEAK_FLOPS, 4)}
    if stock_fits:
        with torch.no_grad():
            a, b = float(M.chamfer_batch(p1, p2)), float(C.stock_chamfer(p1, p2))
        out["value_rel_diff_to_stock"] = abs(a - b) / abs(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="16x4096x4096,16x4096x1024,1x65536x8192,8x65536x65536")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "chamfer", "device": torch.cuda.get_device_name(0), "D": 3, "reps": args.reps, "shapes": {}}
    for s in args.shapes.split(","):
        B, N, Mc = (int(v) for v in s.split("x"))
        res["shapes"][s] = bench_shape(B, N, Mc, args.reps, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
