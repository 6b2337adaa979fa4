#!/usr/bin/env python3
"""Surface normals on the HIP library (``normals.estimate_normals`` = ``pn2_knn`` + ``pn2_local_pca``, and ``normals.local_pca``
alone) against stock torch on the same device, in the same run, alternating.

    python tools/bench_normals.py [--reps 20] [--seed 0] [--only inview,b16x4096,b16x2048]

Prints one JSON line.  Three workloads, synthetic and seeded, a self-search each:

  inview     1 x 28 895 rows, k = 16: a KITTI scan cropped to the camera's view (metres, ground plane plus clutter), radius 1 m
  b16x4096   16 x 4 096 rows, k = 16: a training batch, unit cube
  b16x2048   16 x 2 048 rows, k = 32

  estimate_ms        estimate_normals into normals.buffers: the packed copy, pn2_knn, pn2_local_pca (eager: three launches and a fill)
  estimate_graph_ms  the same, captured once and replayed
  pca_ms             local_pca alone on the neighbour lists of the search (one launch), eager
  pca_graph_ms       the same as a graph replay
  stock_ms           the stock formulation of the whole: expanded-form distances (-2 q.c^T + |q|^2 + |c|^2) in slabs of 8 192 queries,
                     ``topk(k, largest=False)``, the [N, k, 3] gather, the centred ``einsum`` and ``torch.linalg.eigh`` on [N, 3, 3]
  stock_pca_ms       its second half alone: gather, centred einsum, eigh
  cos_median / cos_min   |n_ours . n_stock| over the rows with at least three valid neighbours (the sign is left out; stock takes
                     float32 throughout and applies NO radius, so the two differ on the rows that lose neighbours to the cut-off
                     of `inview`, and where a neighbourhood's two smallest eigenvalues nearly coincide)

Every time is a median of --reps runs (fewer when one run takes more than a second: ``reps_used``) after 2 warm-up runs, host
clock around the device work (a synchronize on either side); ours and stock alternate run by run.
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

from pointnet12_amd import normals as PN              # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating_medians(fns, reps, warmup=2):
    """{name: fn} -> ({name: median ms}, reps used); the functions take turns inside every repetition."""
    slow = 0.0
    for _ in range(warmup):
        for fn in fns.values():
            slow = max(slow, timed(fn))
    reps = max(3, min(reps, int(20e3 / max(slow, 1e-3))))
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return {k: round(float(np.median(v)), 4) for k, v in ms.items()}, reps


def stock_knn(x, k, slab=8192):
    out = []
    x2 = (x * x).sum(-1)
    for n0 in range(0, x.shape[1], slab):
        q = x[:, n0:n0 + slab]
        d = -2.0 * torch.matmul(q, x.transpose(1, 2)) + x2[:, n0:n0 + slab, None] + x2[:, None, :]
        out.append(torch.topk(d, k, dim=-1, largest=False)[1])
    return torch.cat(out, 1)


def stock_pca(x, idx):
    B, N, K = idx.shape
    nb = x[torch.arange(B, device=x.device)[:, None, None], idx]              # [B, N, K, 3]
    c = nb - nb.mean(2, keepdim=True)
    cov = torch.einsum("bnka,bnkc->bnac", c, c) / K
    lam, vec = torch.linalg.eigh(cov)
    return vec[..., 0], lam


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g


def cloud(name, B, M, rng):
    if name == "inview":
        x = np.stack([rng.uniform(2, 60, (B, M)), rng.uniform(-20, 20, (B, M)), rng.normal(-1.6, 0.03, (B, M))], -1)
        up = rng.random((B, M)) < 0.35                            # walls and clutter above the ground plane
        x[..., 2] = np.where(up, rng.uniform(-1.6, 1.5, (B, M)), x[..., 2])
        return x.astype(np.float32)
    return rng.random((B, M, 3), np.float32)


def workload(name, B, M, k, radius, reps, dev, rng):
    x = torch.from_numpy(cloud(name, B, M, rng)).to(dev)
    buf = PN.buffers(M, B=B, k=k, device=dev)
    res = {"B": B, "M": M, "k": k}

    def estimate():
        PN.estimate_normals(x, k=k, radius=radius, viewpoint="origin", return_eig=True, return_count=True, buffers=buf)

    estimate()
    idx, dist = buf.idx.clone(), buf.dist.clone()
    ours = buf.normal.clone()

    def pca():
        PN.local_pca(x, idx, dist, max_dist=radius, viewpoint="origin", return_eig=True, return_count=True, buffers=buf)

    g_est, g_pca = capture(estimate), capture(pca)
    print("%s: captured" % name, file=sys.stderr, flush=True)
    t, used = alternating_medians({"estimate_ms": estimate, "stock_ms": lambda: stock_pca(x, stock_knn(x, k)),
                                   "estimate_graph_ms": g_est.replay}, reps)
    res.update(t)
    print("%s: whole %s" % (name, t), file=sys.stderr, flush=True)
    t2, used2 = alternating_medians({"pca_ms": pca, "stock_pca_ms": lambda: stock_pca(x, idx), "pca_graph_ms": g_pca.replay}, reps)
    res.update(t2)
    res["reps_used"] = [used, used2]
    sn, _ = stock_pca(x, idx)
    ok = buf.count.reshape(B, M) >= 3
    cos = (ours * sn).sum(-1).abs()[ok]
    res["cos_median"] = round(float(cos.median()), 6)
    res["cos_min"] = round(float(cos.min()), 6)
    res["rows_with_fewer_than_3"] = int((~ok).sum())
    for key, stock in (("estimate_ms", "stock_ms"), ("estimate_graph_ms", "stock_ms"), ("pca_ms", "stock_pca_ms"), ("pca_graph_ms", "stock_pca_ms")):
        res["stock_over_" + key[:-3]] = round(res[stock] / res[key], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="inview,b16x4096,b16x2048")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"inview": (1, 28895, 16, 1.0), "b16x4096": (16, 4096, 16, None), "b16x2048": (16, 2048, 32, None)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = workload(name, *shapes[name], args.reps, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
