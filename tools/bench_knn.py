#!/usr/bin/env python3
"""k-nearest-neighbour search and label vote on the HIP library (``pn2_knn``, ``pn2_knn_vote``) against stock torch on the same
device, in the same run.

    python tools/bench_knn.py [--reps 20] [--seed 0] [--only scan,sa,three]

Prints one JSON line.  Three workloads, synthetic and seeded:

  scan    1 x 120 000 queries x 25 000 candidates, K = 5: a KITTI-sized scan (metres) onto its own resample drawn with replacement,
          search and vote (``propagate_labels``'s two launches)
  sa      16 x 1 024 queries x 4 096 candidates, K = 32: a set-abstraction level (``knn_point``)
  three   1 x 4 096 queries x 1 024 candidates, K = 3, beside ``pn2_three_nn``: the same answer, the specialised kernel's time

  knn_ms        pn2_knn into preallocated buffers
  vote_ms       pn2_knn_vote on its result (scan only)
  stock_knn_ms  the stock formulation: the expanded-form distance matrix (-2 q.c^T + |q|^2 + |c|^2, as the reference's
                ``square_distance``) and ``topk(K, largest=False)``; for `scan` in slabs of 8 192 queries (the whole matrix
                would be 12 GB), the slabs' time summed in one timed call
  stock_vote_ms ``torch.mode`` over the gathered labels (scan only; its tie rule is the smallest label, not the nearest voter)
  three_nn_ms   pn2_three_nn (three only)
  idx_equal     fraction of neighbour slots on which stock and pn2_knn agree (they may differ on ties and, in the last bit of a
                distance, through the matrix product's summation order)

Every time is a median of --reps runs after 3 warm-up runs, host clock around the device work (a synchronize on either side).
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

from pointnet12_amd import _lib                       # noqa: E402
from pointnet12_amd import pointnet_util as U         # noqa: E402


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4)


def stock_knn(q, c, K, slab=8192):
    """[B,N,3] x [B,M,3] -> int64 [B,N,K] with stock torch ops."""
    out = []
    c2 = (c * c).sum(-1)[:, None, :]
    for n0 in range(0, q.shape[1], slab):
        qs = q[:, n0:n0 + slab]
        d = -2.0 * torch.matmul(qs, c.transpose(1, 2)) + (qs * qs).sum(-1)[:, :, None] + c2
        out.append(torch.topk(d, K, dim=-1, largest=False)[1])
    return torch.cat(out, 1)


def workload(name, B, N, M, K, reps, dev, rng):
    if name == "scan":
        q = (rng.normal(size=(B, N, 3)) * np.array([25.0, 25.0, 1.5]) + np.array([5.0, 0.0, -1.0])).astype(np.float32)
        c = np.stack([q[b, rng.integers(0, N, M)] for b in range(B)])
    else:
        q = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        c = rng.uniform(-1, 1, (B, M, 3)).astype(np.float32)
    q, c = torch.from_numpy(q).to(dev), torch.from_numpy(np.ascontiguousarray(c)).to(dev)
    idx = torch.empty(B, N, K, device=dev, dtype=torch.int64)
    dist = torch.empty(B, N, K, device=dev, dtype=torch.float32)
    lib, p = _lib.load(), _lib.ptr
    res = {"B": B, "N": N, "M": M, "K": K}

    def knn():
        _lib.check(lib.pn2_knn(p(q), p(c), B, N, M, K, None, None, p(idx), p(dist), _lib.stream()), "pn2_knn")
    res["knn_ms"] = median_ms(knn, reps)
    res["stock_knn_ms"] = median_ms(lambda: stock_knn(q, c, K), reps)
    res["idx_equal"] = round(float((stock_knn(q, c, K) == idx).float().mean()), 6)
    if name == "scan":
        labels = torch.from_numpy(rng.integers(0, 19, (B, M))).to(dev)
        out = torch.empty(B, N, device=dev, dtype=torch.int32)

        def vote():
            _lib.check(lib.pn2_knn_vote(p(idx), p(dist), p(labels), B, N, M, K, float("inf"), None, -1, None, 0, None, N, p(out), None,
                                        _lib.stream()), "pn2_knn_vote")
        res["vote_ms"] = median_ms(vote, reps)
        res["stock_vote_ms"] = median_ms(lambda: torch.mode(torch.gather(labels[:, None, :].expand(B, N, M), 2, idx), -1), reps)
    if name == "three":
        res["three_nn_ms"] = median_ms(lambda: U.three_nn(q, c), reps)
        res["same_as_three_nn"] = bool(torch.equal(U.three_nn(q, c)[0], idx))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="scan,sa,three")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"scan": (1, 120000, 25000, 5), "sa": (16, 1024, 4096, 32), "three": (1, 4096, 1024, 3)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = workload(name, *shapes[name], args.reps, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
