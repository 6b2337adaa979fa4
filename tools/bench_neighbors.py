#!/usr/bin/env python3
"""Grid-accelerated "k nearest within r" (``neighbors.GridIndex`` = ``pn2_grid_build`` + ``pn2_grid_knn``) against the brute force it
replaces (``pn2_knn`` at the same k; the cut-off is applied afterwards by the vote or by ``pn2_local_pca``), on the same device, in
the same run, alternating.

    python tools/bench_neighbors.py [--reps 20] [--seed 0] [--only label,inview,b16x4096,b16x2048,self]

Prints one JSON line.  Workloads, synthetic and seeded:

  label      ``label_scan``'s search: 1 x 120 000 queries (``synthetic.kitti_scan``, metres) x 25 000 candidates drawn from them with
             replacement, K = 5, 1 m
  inview, b16x4096, b16x2048   ``estimate_normals`` on the three clouds of tools/bench_normals.py, the whole call, ``search="brute"``
             against ``search="grid"``.  The two training batches have no radius there; here both sides get one (0.15 / 0.2, about
             1.5 times the distance of the k-th neighbour in a uniform unit cube) so that they compute the same thing
  self       a 120 000-row scan against itself, k = 16, 0.5 m: the grid with and without PN2_GRID_VISIT_SORTED; brute force
             (1.4e10 pairs) three times

  brute_ms / grid_ms          host clock around the device work (a synchronize on either side), medians, the sides taking turns
                              inside every repetition; grid_ms is build plus query
  build_event_ms / query_event_ms   the two halves of the grid side apart, device events, medians
  sorted_ms / unsorted_ms     (self) build plus self-search with and without the flag
  cell_max / cell_mean        the largest and the mean population of the occupied cells (read back outside the timed region)
  idx_equal                   fraction of neighbour slots on which the grid and the brute force (cut applied) agree: they differ only
                              where the difference and the expanded form of the distance disagree on a near-tie or at the cut
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

from pointnet12_amd import _lib, neighbors, synthetic  # noqa: E402
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


def event_median(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 4)


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


def cell_population(x, cell):
    """x [B,M,>=3] on the device -> (largest, mean) population of the occupied cells of a grid of `cell` edges at origin 0."""
    q = torch.floor(x[..., :3].double() / cell).long()
    q = torch.cat([torch.arange(x.shape[0], device=x.device)[:, None, None].expand(-1, x.shape[1], 1), q], -1).reshape(-1, 4)
    pop = torch.unique(q, dim=0, return_counts=True)[1]
    return int(pop.max()), round(float(pop.double().mean()), 2)


def brute_knn(q, c, idx, dist):
    B, N, _ = q.shape
    _lib.check(_lib.load().pn2_knn(_lib.ptr(q), _lib.ptr(c), B, N, c.shape[1], idx.shape[2], None, None, _lib.ptr(idx), _lib.ptr(dist),
                                   _lib.stream()), "pn2_knn")


def agreement(index, gidx, bidx, bdist, M):
    cut = torch.where(bdist > index.max_d2, torch.full_like(bidx, M), bidx)
    return round(float((cut == gidx).float().mean()), 6)


def label_workload(reps, dev, seed):
    N, M, K, radius = 120000, 25000, 5, 1.0
    scan = synthetic.kitti_scan(seed, N)
    rng = np.random.default_rng(seed)
    q = torch.from_numpy(np.ascontiguousarray(scan[None, :, :3])).to(dev)
    c = q[:, torch.from_numpy(rng.integers(0, N, M)).to(dev)].contiguous()
    index = neighbors.GridIndex(radius=radius)
    buf = index.buffers(M, B=1, N=N, k=K)
    bidx, bdist = torch.empty(1, N, K, device=dev, dtype=torch.int64), torch.empty(1, N, K, device=dev, dtype=torch.float32)
    build = lambda: index.build(c, buffers=buf)
    query = lambda: index.query(q, K, return_dist=True, return_count=True, buffers=buf)
    res = {"N": N, "M": M, "K": K, "radius": radius}
    t, used = alternating_medians({"brute_ms": lambda: brute_knn(q, c, bidx, bdist), "grid_ms": lambda: (build(), query())}, reps)
    res.update(t)
    res["reps_used"] = used
    res["build_event_ms"], res["query_event_ms"] = event_median(build, reps), event_median(query, reps)
    res["cell_max"], res["cell_mean"] = cell_population(c, index.cell[0])
    res["idx_equal"] = agreement(index, buf.idx, bidx, bdist, M)
    res["mean_in_radius"] = round(float(buf.count.float().mean()), 2)
    res["brute_over_grid"] = round(res["brute_ms"] / res["grid_ms"], 2)
    return res


def normals_cloud(name, B, M, rng):
    """The clouds of tools/bench_normals.py."""
    if name == "inview":
        x = np.stack([rng.uniform(2, 60, (B, M)), rng.uniform(-20, 20, (B, M)), rng.normal(-1.6, 0.03, (B, M))], -1)
        up = rng.random((B, M)) < 0.35
        x[..., 2] = np.where(up, rng.uniform(-1.6, 1.5, (B, M)), x[..., 2])
        return x.astype(np.float32)
    return rng.random((B, M, 3), np.float32)


def normals_workload(name, B, M, k, radius, reps, dev, rng):
    x = torch.from_numpy(normals_cloud(name, B, M, rng)).to(dev)
    bufs = {s: PN.buffers(M, B=B, k=k, device=dev, search=s) for s in ("brute", "grid")}
    res = {"B": B, "M": M, "k": k, "radius": radius}

    def estimate(search):
        return lambda: PN.estimate_normals(x, k=k, radius=radius, viewpoint="origin", return_eig=True, return_count=True,
                                           buffers=bufs[search], search=search)

    graphs = {s: capture(estimate(s)) for s in bufs}
    t, used = alternating_medians({"brute_ms": estimate("brute"), "grid_ms": estimate("grid"), "brute_graph_ms": graphs["brute"].replay,
                                   "grid_graph_ms": graphs["grid"].replay}, reps)
    res.update(t)
    res["reps_used"] = used
    index = neighbors.GridIndex(radius=radius)
    res["build_event_ms"] = event_median(lambda: index.build(x, buffers=bufs["grid"].grid), reps)
    res["query_event_ms"] = event_median(lambda: index.query_self(k, return_dist=True, buffers=bufs["grid"].grid), reps)
    res["cell_max"], res["cell_mean"] = cell_population(x, index.cell[0])
    estimate("brute")(), estimate("grid")()
    res["idx_equal"] = agreement(index, bufs["grid"].idx, bufs["brute"].idx, bufs["brute"].dist, M)
    res["normals_equal"] = round(float((bufs["grid"].normal == bufs["brute"].normal).all(-1).float().mean()), 6)
    res["brute_over_grid"] = round(res["brute_ms"] / res["grid_ms"], 2)
    res["brute_over_grid_graph"] = round(res["brute_graph_ms"] / res["grid_graph_ms"], 2)
    return res


def self_workload(reps, dev, seed):
    M, k, radius = 120000, 16, 0.5
    x = torch.from_numpy(synthetic.kitti_scan(seed + 1, M)[None]).to(dev)          # [1, M, 4], read where it lies
    index = neighbors.GridIndex(radius=radius)
    buf = index.buffers(M, B=1, k=k)
    build = lambda: index.build(x, buffers=buf)
    search = lambda s: (lambda: index.query_self(k, return_dist=True, return_count=True, visit_sorted=s, buffers=buf))
    res = {"M": M, "k": k, "radius": radius}
    t, used = alternating_medians({"sorted_ms": lambda: (build(), search(True)()), "unsorted_ms": lambda: (build(), search(False)())}, reps)
    res.update(t)
    res["reps_used"] = used
    res["build_event_ms"] = event_median(build, reps)
    res["query_sorted_event_ms"], res["query_unsorted_event_ms"] = event_median(search(True), reps), event_median(search(False), reps)
    res["cell_max"], res["cell_mean"] = cell_population(x, index.cell[0])
    res["mean_in_radius"] = round(float(buf.count.float().mean()), 2)
    xyz = x[..., :3].contiguous()
    bidx, bdist = torch.empty(1, M, k, device=dev, dtype=torch.int64), torch.empty(1, M, k, device=dev, dtype=torch.float32)
    res["brute_ms"] = round(float(np.median([timed(lambda: brute_knn(xyz, xyz, bidx, bdist)) for _ in range(3)])), 4)
    search(True)()
    res["idx_equal"] = agreement(index, buf.idx, bidx, bdist, M)
    res["unsorted_over_sorted"] = round(res["unsorted_ms"] / res["sorted_ms"], 2)
    res["brute_over_grid"] = round(res["brute_ms"] / min(res["sorted_ms"], res["unsorted_ms"]), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="label,inview,b16x4096,b16x2048,self")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"inview": (1, 28895, 16, 1.0), "b16x4096": (16, 4096, 16, 0.15), "b16x2048": (16, 2048, 32, 0.2)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "self_visit_sorted_default": neighbors.SELF_VISIT_SORTED}
    for name in args.only.split(","):
        if name == "label":
            out[name] = label_workload(args.reps, dev, args.seed)
        elif name == "self":
            out[name] = self_workload(args.reps, dev, args.seed)
        else:
            out[name] = normals_workload(name, *shapes[name], args.reps, dev, rng)
        print("%s: %s" % (name, out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
