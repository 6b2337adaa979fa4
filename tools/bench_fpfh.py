#!/usr/bin/env python3
"""FPFH descriptors on the HIP library (``features.compute_fpfh`` = normals + grid search + ``pn2_spfh`` + ``pn2_fpfh``, and the two
kernels alone) against the same descriptor in stock torch on the same device, in the same run, alternating.

    python tools/bench_fpfh.py [--reps 20] [--seed 0] [--only inview,b16x4096,sheets]

Prints one JSON line.  Two timed workloads, synthetic and seeded, a self-search each, and one sanity figure:

  inview     1 x 28 895 rows, k = 32, radius 1 m: a KITTI scan cropped to the camera's view (metres, ground plane plus clutter)
  b16x4096   16 x 4 096 rows, k = 32, radius 0.15: a training batch, unit cube
  sheets     tests/icp_ref.py's wavy-sheet pair (1 024 source rows of a 2 048-row target, 3 degrees about (1, 2, 3) plus a
             translation), radius 0.5: ``match_share`` = the share of source rows whose nearest target row in FEATURE space
             (``torch.cdist`` here, on the 33 numbers alone) lies within 2 x radius of the row's true position.  No threshold.

  spfh_ms            pn2_spfh alone on the neighbour lists and normals of the whole (one launch), eager
  fpfh_ms            pn2_fpfh alone on those SPFH rows (one launch), eager
  descr_ms           both (``features.fpfh`` into ``features.buffers``: two launches and a fill)
  descr_graph_ms     the same as a graph replay
  stock_ms           the stock formulation of the same rule on the same lists, fp64: the [N, k, 3] gathers of neighbours and their
                     normals, the pair features vectorised over [N, k], three ``scatter_add_`` into [N, 33], the [N, k, 33] gather
                     of the neighbours' histograms and the weighted sum
  compute_ms         the whole ``compute_fpfh`` (estimate_normals with search="grid", the grid build and self-search, both kernels), eager
  compute_graph_ms   the same, captured once and replayed
  rows_equal / max_abs_diff   how the two descriptors agree: the share of rows whose 33 integer counts are equal, and the largest
                     difference of the float32 results (torch's atan2 and its order of summation are its own)

Every time is a median of --reps runs (fewer when one run takes more than a second: ``reps_used``) after 2 warm-up runs, host
clock around the device work (a synchronize on either side); ours and stock alternate run by run.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                          # noqa: E402

from pointnet12_amd import features as FT             # noqa: E402


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


def _dot(a, b):
    return (a * b).sum(-1)


def stock_fpfh(x, nrm, idx, max_d2):
    """The rule of include/pn2.h ("FPFH") in stock torch, fp64: x, nrm [B,M,3] float32, idx [B,M,K] -> (fpfh float32 [B,M,33],
    counts [B,M,33], m [B,M])."""
    B, M, K = idx.shape
    bi = torch.arange(B, device=x.device)[:, None, None]
    inr = (idx >= 0) & (idx < M)
    j = idx.clamp(0, M - 1)
    xd, nd = x.double(), nrm.double()
    dp = xd[bi, j] - xd[:, :, None, :]
    ni, nj = nd[:, :, None, :].expand(B, M, K, 3), nd[bi, j]
    d2 = _dot(dp, dp)
    geo = inr & (d2 > 0) & (d2 <= max_d2)
    d = d2.sqrt()
    a1, a2 = _dot(ni, dp) / d, _dot(nj, dp) / d
    on_j = (a1.abs() < a2.abs())[..., None]
    ns, nt = torch.where(on_j, nj, ni), torch.where(on_j, ni, nj)
    dp = torch.where(on_j, -dp, dp)
    f3 = torch.where(on_j[..., 0], -a2, a1)
    v = torch.cross(dp, ns, dim=-1)
    vl = _dot(v, v).sqrt()
    pair = geo & (vl > 0) & (ni != 0).any(-1) & (nj != 0).any(-1)
    v = v / vl[..., None]
    w = torch.cross(ns, v, dim=-1)
    f2 = _dot(v, nt)
    f1 = torch.atan2(_dot(w, nt) + 0.0, _dot(ns, nt))
    t = torch.stack([11.0 * (f1 + math.pi) / (2.0 * math.pi), 11.0 * (f2 + 1.0) * 0.5, 11.0 * (f3 + 1.0) * 0.5], -1)
    bins = torch.nan_to_num(t, nan=0.0).floor().clamp(0, 10).long() + torch.tensor([0, 11, 22], device=x.device)
    hist = torch.zeros(B * M, 33, device=x.device, dtype=torch.float64)
    one = pair.reshape(B * M, K).double()
    for a in range(3):
        hist.scatter_add_(1, bins[..., a].reshape(B * M, K), one)
    hist = hist.reshape(B, M, 33)
    m = pair.sum(-1)
    s = torch.where(m[..., None] > 0, 100.0 * hist / m[..., None].clamp(min=1), torch.zeros_like(hist))
    wgt = torch.where(geo & (m[bi, j] > 0), 1.0 / d2, torch.zeros_like(d2))
    A = (s[bi, j] * wgt[..., None]).sum(2)
    W = wgt.sum(-1, keepdim=True)
    f = s + torch.where(W > 0, A / W.clamp(min=1e-300), torch.zeros_like(A))
    return f.float(), hist, m


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
    buf = FT.buffers(M, B=B, k=k, device=dev, search="grid")
    res = {"B": B, "M": M, "k": k, "radius": radius}

    def compute():
        FT.compute_fpfh(x, radius, k=k, viewpoint="origin", buffers=buf)

    compute()
    idx, nrm, spfh_rows = buf.idx.clone(), buf.normals.normal.clone(), buf.spfh.clone()
    ours = buf.fpfh.clone()
    out = torch.empty_like(ours)
    max_d2 = float(np.float32(radius ** 2))
    lib, p = FT._lib.load(), FT._p

    def spfh():
        FT.spfh(x, nrm, idx, max_dist=radius, buffers=buf)

    def fpfh():
        FT._lib.check(lib.pn2_fpfh(p(x), 3, p(idx), p(spfh_rows), B, M, k, max_d2, None, p(out), None, FT._lib.stream()), "pn2_fpfh")

    def descr():
        FT.fpfh(x, nrm, idx, max_dist=radius, buffers=buf)

    g_compute, g_descr = capture(compute), capture(descr)
    print("%s: captured" % name, file=sys.stderr, flush=True)
    t, used = alternating_medians({"descr_ms": descr, "stock_ms": lambda: stock_fpfh(x, nrm, idx, max_d2), "descr_graph_ms": g_descr.replay,
                                   "spfh_ms": spfh, "fpfh_ms": fpfh}, reps)
    res.update(t)
    print("%s: descriptor %s" % (name, t), file=sys.stderr, flush=True)
    t2, used2 = alternating_medians({"compute_ms": compute, "compute_graph_ms": g_compute.replay}, reps)
    res.update(t2)
    res["reps_used"] = [used, used2]
    sf, hist, m = stock_fpfh(x, nrm, idx, max_d2)
    counts, _ = FT.spfh_counts(spfh_rows)
    res["rows_equal"] = round(float((counts.double() == hist).all(-1).double().mean()), 6)
    res["max_abs_diff"] = round(float((sf - ours).abs().max()), 6)
    res["rows_without_a_pair"] = int((m == 0).sum())
    for key in ("descr_ms", "descr_graph_ms"):
        res["stock_over_" + key[:-3]] = round(res["stock_ms"] / res[key], 2)
    return res


def sheets(dev):
    """The sanity figure: see the module docstring."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import icp_ref
    src, tgt, _ = icp_ref.sheets_pair()
    radius = 0.5
    eye = np.array([0.0, 0.0, 8.0])
    eye_src = (eye - icp_ref.PLANTED_T) @ icp_ref.PLANTED_R               # the viewpoint moves with the cloud
    ft = FT.compute_fpfh(torch.from_numpy(np.array(tgt[0])).to(dev), radius, k=32, viewpoint=eye.tolist())
    fs = FT.compute_fpfh(torch.from_numpy(np.array(src[0])).to(dev), radius, k=32, viewpoint=eye_src.tolist())
    nn = torch.cdist(fs, ft).argmin(1).cpu().numpy()
    true = tgt[0][::2].astype(np.float64)
    off = np.linalg.norm(tgt[0][nn].astype(np.float64) - true, axis=1)
    return {"N": int(len(true)), "M": int(tgt.shape[1]), "radius": radius, "match_share": round(float((off <= 2 * radius).mean()), 4),
            "exact_share": round(float((nn == 2 * np.arange(len(true))).mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="inview,b16x4096,sheets")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"inview": (1, 28895, 32, 1.0), "b16x4096": (16, 4096, 32, 0.15)}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = sheets(dev) if name == "sheets" else workload(name, *shapes[name], args.reps, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
