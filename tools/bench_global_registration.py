#!/usr/bin/env python3
"""Global registration on the HIP library (``registration.register_global`` = FPFH on both clouds + ``features.match_features`` +
``registration.ransac_correspondences``) and its matching kernel against stock torch on the same device, in the same run, alternating.

    python tools/bench_global_registration.py [--reps 20] [--only bumps3k,bumps24k,estimated]

Prints one JSON line.  The scene is tests/corr_ransac_ref.py's ``bump_scene`` (two overlapping, differently posed parts of a height
field of Gaussian bumps, analytic normals): ``bumps3k`` is the end-to-end test's (3 072 points: N = 2 199 source, M = 2 127 target
rows), ``bumps24k`` the same surface with 24 576 points.  k = 32, radius = 0.35 (0.15 at 24k), threshold = 0.05 (0.02), the
normals passed in, search = "brute" at 3k and "grid" at 24k.

  nn2_ms             pn2_feature_nn2 alone: the two nearest of M target descriptors for each of N source descriptors (one launch)
  stock_nn2_ms       ``torch.cdist(fs, ft).topk(2, largest=False)`` on the same descriptors
  nearest_equal      the share of source rows (among those that take part) on whose nearest target row the two agree (cdist works
                     from |a|^2 + |b|^2 - 2ab: its distances are not the separately rounded sums, near-ties may resolve differently)
  stock_pick_within_1e-3   the share of those rows on which the row cdist picked is, by the exact fp64 distance, no further than
                     1.001 times the row the kernel picked (1.0: every disagreement is a near-tie)
  match_ms           the whole ``match_features`` (mutual, ratio 0.9: two searches and the compaction) into its buffers
  ransac_ms          ``ransac_correspondences`` on those pairs (1 024 hypotheses, two refits, the closing evaluation) into its buffers
  global_ms          the whole ``register_global`` with buffers, eager
  global_graph_ms    the same, captured once and replayed
  pairs / inliers / row_error   of that call: the pair list's length, the inliers of the result, the largest distance of a source
                     row moved by the result from its true position

``estimated`` is a sanity figure without a threshold: the 3k scene through ``compute_fpfh``'s OWN normals (each cloud oriented
towards a viewpoint 10 above the surface, moved with the cloud) and the grid search: pairs, inliers and row_error of one call.

Every time is a median of --reps runs after 2 warm-up runs, host clock around the device work (a synchronize on either side); ours
and stock alternate run by run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                          # noqa: E402

import corr_ransac_ref as C                           # noqa: E402
from pointnet12_amd import features as FT             # noqa: E402
from pointnet12_amd import registration as RG         # noqa: E402


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


def row_error(transform, sc):
    moved = C.apply(transform.cpu().numpy()[:3].reshape(12), sc["source"].astype(np.float64))
    return float(np.linalg.norm(moved - sc["truth"], axis=1).max())


def workload(points, radius, threshold, search, reps, dev):
    sc = C.bump_scene(points)
    src, tgt, ns, nt = (torch.from_numpy(np.array(sc[k])).to(dev)[None] for k in ("source", "target", "source_normals", "target_normals"))
    N, M, k = src.shape[1], tgt.shape[1], 32
    res = {"N": N, "M": M, "k": k, "radius": radius, "threshold": threshold, "search": search}
    buf = RG.global_buffers(N, M, B=1, k=k, iterations=1024, device=dev, search=search)

    def whole():
        return RG.register_global(src, tgt, radius, threshold=threshold, k=k, normals=(ns, nt), search=search, buffers=buf)

    out = whole()
    fs, ft = buf.source_fpfh.fpfh.clone(), buf.target_fpfh.fpfh.clone()
    res.update(pairs=int(out.matches.count), inliers=int(out.count), row_error=round(row_error(out.transform[0], sc), 6), status=int(out.status))
    idx, dist = torch.empty(1, N, 2, device=dev, dtype=torch.int64), torch.empty(1, N, 2, device=dev)
    lib, p = FT._lib.load(), FT._p

    def nn2():
        FT._lib.check(lib.pn2_feature_nn2(p(fs), 33, p(ft), 33, 1, N, M, 33, None, None, p(idx), p(dist), FT._lib.stream()), "pn2_feature_nn2")

    def stock_nn2():
        return torch.cdist(fs, ft).topk(2, largest=False)

    def match():
        return FT.match_features(fs, ft, buffers=buf.matches)

    def ransac():
        return RG.ransac_correspondences(src, tgt, match_res, threshold, buffers=buf.corr)

    match_res = match()
    g = capture(whole)
    t, used = alternating_medians({"nn2_ms": nn2, "stock_nn2_ms": stock_nn2, "match_ms": match, "ransac_ms": ransac}, reps)
    res.update(t)
    t2, used2 = alternating_medians({"global_ms": whole, "global_graph_ms": g.replay}, reps)
    res.update(t2)
    res["reps_used"] = [used, used2]
    nn2()
    part = idx[0, :, 0] < M
    res["rows_that_take_part"] = int(part.sum())
    pick = stock_nn2()[1][0, :, 0]
    res["nearest_equal"] = round(float((pick == idx[0, :, 0])[part].double().mean()), 6)
    d_ours = (fs[0].double() - ft[0, idx[0, :, 0].clamp(max=M - 1)].double()).pow(2).sum(1)
    d_pick = (fs[0].double() - ft[0, pick].double()).pow(2).sum(1)
    res["stock_pick_within_1e-3"] = round(float((d_pick <= d_ours * (1.0 + 1e-3))[part].double().mean()), 6)
    res["stock_over_nn2"] = round(res["stock_nn2_ms"] / res["nn2_ms"], 2)
    return res


def estimated(dev):
    """The sanity figure: see the module docstring."""
    sc = C.bump_scene()
    src, tgt = (torch.from_numpy(np.array(sc[k])).to(dev) for k in ("source", "target"))
    T = sc["T_true"].reshape(3, 4)
    eye = np.array([0.0, 0.0, 10.0])
    eye_src = (eye - T[:, 3]) @ T[:, :3]                            # the viewpoint moves with the cloud: T^-1 eye
    out = RG.register_global(src, tgt, 0.35, threshold=0.05, k=32, search="grid", viewpoint=(eye_src.tolist(), eye.tolist()))
    return {"N": int(src.shape[0]), "M": int(tgt.shape[0]), "pairs": int(out.matches.count), "inliers": int(out.count), "status": int(out.status),
            "row_error": round(row_error(out.transform, sc), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="bumps3k,bumps24k,estimated")
    args = ap.parse_args()
    dev = torch.device("cuda")
    shapes = {"bumps3k": (3072, 0.35, 0.05, "brute"), "bumps24k": (24576, 0.15, 0.02, "grid")}
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = estimated(dev) if name == "estimated" else workload(*shapes[name], args.reps, dev)
        print("%s: %s" % (name, out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
