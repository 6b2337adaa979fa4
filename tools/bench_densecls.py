#!/usr/bin/env python3
"""PointNetDenseCls (ShapeNet part segmentation) on the HIP library against stock PyTorch, on one GPU.

    python tools/bench_densecls.py [--reps 20] [--no-profile]

Prints one JSON line:
  densecls_step_ms        training step (forward + backward, default PointNetLoss) of PointNetDenseCls() at B = 16 x 2048 (partseg.py)
  densecls_step_torch_ms  the same step of the fp32 stock-torch restatement in the reference's formulation (torch.bmm transforms, the
                          materialised [B, N, 4944] concatenation; tests/densecls_ref.py), same GPU, same process
  densecls_eval_ms        PointNetDenseCls().eval() under no_grad on one 2048-point cloud
  convs1_fwd_us / _tflops      pn2_conv1x1_fwd_multi at the step's shape (32 768 x 2880 -> 256 over the five sources, 48.3 GFLOP)
  convs1_wgrad_us / _tflops    pn2_conv1x1_wgrad_multi at that shape (device time between events, mean over --reps calls)
  top_kernels             the kernels with the most device time per library step, from ONE separate
                          `rocprofv3 --kernel-trace --stats` run of this script (no counter collection); omitted with --no-profile
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                          # noqa: E402

from pointnet12_amd import _lib as L                  # noqa: E402
from pointnet12_amd import pointnet as M              # noqa: E402
import densecls_ref as D                              # noqa: E402
import pointnet_v1_ref as V                           # noqa: E402

B, N = 16, 2048


def timeit(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def setup(dev):
    torch.manual_seed(0)
    net = M.PointNetDenseCls().to(dev).train()
    gen = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(B, 3, N, generator=gen).to(dev)
    cls = torch.randint(0, 16, (B,), generator=gen).to(dev)
    seg = torch.randint(0, 50, (B, N), generator=gen).to(dev)
    return net, x, cls, seg, torch.eye(16, device=dev)[cls]


def lib_step(net, x, cls, seg, onehot):
    crit = M.PointNetLoss()

    def step():
        net.zero_grad(set_to_none=True)
        n, n2, tf = net(x, onehot)
        crit(n, cls, n2.contiguous().view(-1, 50), seg.view(-1), tf)[0].backward()
    return step


def gemm_rates(dev, reps):
    """convs1's per-point GEMMs alone at the step's shape: (fwd us, fwd TF/s, wgrad us, wgrad TF/s)."""
    lib, st = L.load(), L.stream()
    P = B * N
    gen = torch.Generator(device="cpu").manual_seed(5)
    ks = (64, 128, 128, 512, 2048)
    srcs = [torch.randn(P, k, generator=gen).to(dev) for k in ks]
    aff = torch.zeros(4 * 2048, device=dev)
    aff[2048:4096] = 1.0
    table = L.src_table([(s.data_ptr(), s.shape[1], s.shape[1], None, 0) for s in srcs[:4]] + [(srcs[4].data_ptr(), 2048, 2048, aff.data_ptr(), 0)])
    W = (torch.randn(256, 4944, generator=gen) / 70).to(dev)
    b = torch.zeros(256, device=dev)
    gb = torch.randn(B, 256, generator=gen).to(dev)
    Y = torch.empty(P, 256, device=dev)
    stats = torch.zeros(8 * 2 * 256, device=dev, dtype=torch.float64)
    dZ = torch.randn(P, 256, generator=gen).to(dev)
    coef = torch.zeros(4 * 256, device=dev)
    coef[:256] = 1.0
    dW = torch.zeros(256, 4944, device=dev)
    flop = 2.0 * P * 2880 * 256

    def fwd():
        L.check(lib.pn2_conv1x1_fwd_multi(table, 5, W.data_ptr() + 4 * 2064, 4944, b.data_ptr(), gb.data_ptr(), 256, N, Y.data_ptr(), 256, P,
                                          256, stats.data_ptr(), st), "pn2_conv1x1_fwd_multi")

    def wgrad():
        L.check(lib.pn2_conv1x1_wgrad_multi(dZ.data_ptr(), 256, Y.data_ptr(), 256, coef.data_ptr(), table, 5, dW.data_ptr() + 4 * 2064, 4944,
                                            None, P, 256, st), "pn2_conv1x1_wgrad_multi")
    out = []
    for fn in (fwd, wgrad):
        for _ in range(3):
            fn()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(e) * 1e3 / reps
        out += [round(us, 1), round(flop / (us * 1e-6) / 1e12, 1)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=0, help=argparse.SUPPRESS)   # (the child of the rocprofv3 run)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    net, x, cls, seg, onehot = setup(dev)
    if args.profile_steps:
        step = lib_step(net, x, cls, seg, onehot)
        for _ in range(args.profile_steps):
            step()
        torch.cuda.synchronize()
        return
    res = {"metric": "pointnet_densecls", "device": torch.cuda.get_device_name(0)}
    res["densecls_step_ms"] = round(timeit(lib_step(net, x, cls, seg, onehot), args.reps), 3)

    P = V.Params(net.state_dict(), torch.float32, dev)

    def torch_step():
        for v in P.p.values():
            v.grad = None
        n, n2, _, tf = D.dense_forward(P, x, onehot, True, "concat")
        D.dense_loss(n, cls, n2, seg, tf)[0].backward()
    res["densecls_step_torch_ms"] = round(timeit(torch_step, args.reps), 3)
    del P
    torch.cuda.empty_cache()

    torch.manual_seed(0)
    enet = M.PointNetDenseCls().to(dev).eval()
    cloud = torch.randn(1, 3, N, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)

    def infer():
        with torch.no_grad():
            enet(cloud, onehot[:1])
    res["densecls_eval_ms"] = round(timeit(infer, args.reps), 3)
    res["convs1_fwd_us"], res["convs1_fwd_tflops"], res["convs1_wgrad_us"], res["convs1_wgrad_tflops"] = gemm_rates(dev, args.reps)

    if not args.no_profile and shutil.which("rocprofv3"):
        res["top_kernels"] = profile()
    print(json.dumps(res))


def profile(steps=10, top=12):
    """One rocprofv3 --kernel-trace --stats run of `steps` library steps in a child process: [(kernel, us per step, calls per step)]."""
    d = tempfile.mkdtemp(prefix="pn1d_prof_")
    try:
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--profile-steps", str(steps)]
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            return {"error": "rocprofv3 exit %d" % r.returncode}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        rows = list(csv.DictReader(open(files[0])))
        rows.sort(key=lambda r: -float(r.get("TotalDurationNs", 0)))
        return [(r["Name"][:120], round(float(r["TotalDurationNs"]) / 1e3 / steps, 1), int(r.get("Calls", 0)) // steps)
                for r in rows[:top]]
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
