#!/usr/bin/env python3
"""``registration.icp`` (``pn2_grid_build`` + 30 x ``pn2_icp_step`` + the closing evaluation) against the same point-to-plane
iteration in stock torch on the same device, in the same run, alternating; eager and as a graph replay.

    python tools/bench_registration.py [--reps 20] [--seed 0] [--only scan,b16x4096]

Prints one JSON line.  No threshold is attached: the numbers are a record.  Workloads, synthetic and seeded:

  scan       a ``synthetic.kitti_scan`` scan of 120 000 rows and the same scene seen from 0.5 m and 1 degree of yaw away (rows shuffled); the target
             is voxel-downsampled at 0.2 m (dense ground rings make 1 m cells slow -- README.md, grid kNN -- which is why), max_dist
             1 m, 30 iterations, normals from ``estimate_normals`` outside the timed region
  b16x4096   16 x 4 096 unit-cube clouds against themselves moved by 0.02 and 1 degree, max_dist 0.1

The stock side per iteration: the fp64 transform, float32 expanded-form distances in slabs of 8 192 queries, ``argmin``, the mask
``d2 <= max_d2``, the residual and Jacobian of every row, ``J.T @ J``, ``torch.linalg.solve``, Rodrigues; it has no convergence test and
always does all 30 (its replay uses ``torch.linalg.solve_ex``: ``solve`` checks its result on the host and cannot be captured; where
that cannot be captured either the stock replay is reported as null).  Ours is timed twice: ``icp_ms`` with the default tolerances (a converged cloud is frozen, its later steps return
at once) and ``icp_full_ms`` with tolerance 0 (all 30 steps walk).

  *_ms                 host clock around the device work (a synchronize on either side), medians, the sides taking turns inside
                       every repetition;  *_graph_ms: the same as a graph replay
  iterations / fitness / rmse   of the default-tolerance run;  dT_stock: the largest entry of |T_ours - T_stock|
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

from pointnet12_amd import registration, synthetic, voxel  # noqa: E402
from pointnet12_amd import normals as PN              # noqa: E402

SLAB = 8192


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


def yaw_transform(deg, t):
    a = np.radians(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


def stock_icp(src, tgt, nrm, max_d2, iterations, out, solve=torch.linalg.solve):
    """src [B,N,3], tgt [B,M,3], nrm [B,M,3] float32 -> out [B,3,4] float64: point-to-plane Gauss-Newton in stock torch."""
    B, N, _ = src.shape
    s = src.double()
    R = torch.eye(3, device=src.device, dtype=torch.float64).expand(B, 3, 3).contiguous()
    t = torch.zeros(B, 3, device=src.device, dtype=torch.float64)
    c2 = (tgt * tgt).sum(-1)
    rows = torch.arange(B, device=src.device)[:, None]
    eye = torch.eye(3, device=src.device, dtype=torch.float64)
    for _ in range(iterations):
        p = s @ R.transpose(1, 2) + t[:, None, :]
        q = p.float()
        j = torch.empty(B, N, device=src.device, dtype=torch.int64)
        d2 = torch.empty(B, N, device=src.device, dtype=torch.float32)
        for a in range(0, N, SLAB):
            qs = q[:, a:a + SLAB]
            d = (qs * qs).sum(-1)[:, :, None] + c2[:, None, :] - 2.0 * (qs @ tgt.transpose(1, 2))
            d2[:, a:a + SLAB], j[:, a:a + SLAB] = d.min(-1)
        w = (d2 <= max_d2).double()
        n = nrm[rows, j].double()
        e = p - tgt[rows, j].double()
        r = (n * e).sum(-1) * w
        J = torch.cat([torch.linalg.cross(p, n), n], -1) * w[..., None]
        x = solve(J.transpose(1, 2) @ J, -(J.transpose(1, 2) @ r[..., None]))[..., 0]
        om, th = x[:, :3], x[:, :3].norm(dim=-1).clamp(min=1e-30)[:, None, None]
        K = torch.zeros(B, 3, 3, device=src.device, dtype=torch.float64)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -om[:, 2], om[:, 1], om[:, 2], -om[:, 0], -om[:, 1], om[:, 0]
        D = eye + torch.sin(th) / th * K + (1 - torch.cos(th)) / (th * th) * (K @ K)
        R, t = D @ R, (D @ t[..., None])[..., 0] + x[:, 3:]
    out[:, :, :3], out[:, :, 3] = R, t
    return out


def workload(src, tgt, max_dist, reps):
    """src [B,N,ld], tgt [B,M,ld] on the device."""
    B, N, _ = src.shape
    M, dev = tgt.shape[1], src.device
    nrm = PN.estimate_normals(tgt, k=16, radius=2.0 * max_dist, search="grid").contiguous()
    buf = registration.buffers(N, M, B, device=dev, normals=False)
    src3, tgt3 = src[..., :3].contiguous(), tgt[..., :3].contiguous()
    stock_T = torch.zeros(B, 3, 4, device=dev, dtype=torch.float64)
    max_d2 = float(np.float32(max_dist ** 2))
    ours = lambda: registration.icp(src, tgt, max_dist, target_normals=nrm, iterations=30, buffers=buf)
    full = lambda: registration.icp(src, tgt, max_dist, target_normals=nrm, iterations=30, tol_rot=0.0, tol_trans=0.0, buffers=buf)
    stock = lambda: stock_icp(src3, tgt3, nrm, max_d2, 30, stock_T)
    res = {"B": B, "N": N, "M": M, "max_dist": max_dist}
    t, used = alternating_medians({"icp_ms": ours, "icp_full_ms": full, "stock_ms": stock}, reps)
    res.update(t)
    res["reps_used"] = used
    graphs = {"icp_graph_ms": capture(ours).replay, "icp_full_graph_ms": capture(full).replay}
    res.update(alternating_medians(graphs, reps)[0])
    # torch.linalg.solve checks its result on the host and cannot be captured; solve_ex does not check, and is tried LAST: if this
    # build's solver cannot be captured either, the stock replay is reported as null and everything above stands
    res["stock_graph_ms"] = None
    try:
        graphs["stock_graph_ms"] = capture(lambda: stock_icp(src3, tgt3, nrm, max_d2, 30, stock_T, lambda A, b: torch.linalg.solve_ex(A, b)[0])).replay
        res.update(alternating_medians(graphs, reps)[0])
    except Exception as exc:                                          # (a refusal to capture, not a failure of the run)
        res["stock_graph_error"] = str(exc).splitlines()[0][:120]
        torch.cuda.synchronize()
    stock()
    r = ours()
    res["iterations"] = r.iterations.tolist()
    res["fitness"] = [round(v, 4) for v in r.fitness.tolist()]
    res["rmse"] = [round(v, 5) for v in r.rmse.tolist()]
    res["status"] = r.status.tolist()
    res["dT_stock"] = float((r.transform[:, :3] - stock_T).abs().max())
    res["stock_over_icp"] = round(res["stock_ms"] / res["icp_ms"], 2)
    res["stock_over_icp_full"] = round(res["stock_ms"] / res["icp_full_ms"], 2)
    if res["stock_graph_ms"] is not None:
        res["stock_over_icp_full_graph"] = round(res["stock_graph_ms"] / res["icp_full_graph_ms"], 2)
    return res


def scan_workload(reps, dev, seed):
    n = 120000
    move = yaw_transform(1.0, (0.5, 0.0, 0.0))
    first = torch.from_numpy(synthetic.kitti_scan(seed, n)).to(dev)
    second = first.clone()                                          # the same scene seen from 0.5 m and 1 degree away ...
    second[:, :3] = registration.transform_points(first, torch.from_numpy(np.linalg.inv(move)).to(dev))
    second = second[torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))[:n // 2 * 2]]
    down = voxel.VoxelGrid(0.2, device=dev).downsample(first)
    target = down[0][:int(down[3].sum().item())].contiguous()       # ... against the first, downsampled at 0.2 m
    res = workload(second[None].contiguous(), target[None], 1.0, reps)
    res["voxel"] = 0.2
    return res


def cube_workload(reps, dev, rng):
    tgt = torch.from_numpy(rng.random((16, 4096, 3), np.float32)).to(dev)
    move = yaw_transform(1.0, (0.02, -0.01, 0.015))
    src = registration.transform_points(tgt, torch.from_numpy(np.linalg.inv(move)).to(dev)).contiguous()
    return workload(src, tgt, 0.1, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="scan,b16x4096")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = scan_workload(args.reps, dev, args.seed) if name == "scan" else cube_workload(args.reps, dev, rng)
        print("%s: %s" % (name, out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
