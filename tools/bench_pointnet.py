#!/usr/bin/env python3
"""PointNet v1 on the HIP library (pointnet12_amd/pointnet.py) against stock PyTorch, on one GPU.

    python tools/bench_pointnet.py [--reps 20] [--no-profile]

Prints one JSON line:
  seg_step_ms        training step (forward + backward, loss nll + 0.001 reg) of PointNetSeg(13, 9, True) at B = 16 x 4096 (S3DIS)
  seg_step_torch_ms  the same step of the fp32 stock-torch restatement in the reference's formulation (torch.bmm transforms, the
                     materialised [B, N, 1088] concatenation; tests/pointnet_v1_ref.py)
  seg_eval_ms        PointNetSeg(19, 4, True).eval() under no_grad on one 25 000-point cloud (the viewer's shape)
  cls_step_ms        training step of PointNetCls(40, True) at B = 16 x 1024
  top_kernels        the kernels with the most device time over `--profile-steps` library Seg steps, from ONE separate
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
import torch.nn.functional as F                       # noqa: E402

from pointnet12_amd import pointnet as M              # noqa: E402
import pointnet_v1_ref as V                           # noqa: E402


def timeit(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def seg_setup(dev, B=16, N=4096):
    torch.manual_seed(0)
    net = M.PointNetSeg(13, 9, True).to(dev).train()
    gen = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(B, 9, N, generator=gen).to(dev)
    labels = torch.randint(0, 13, (B, N), generator=gen).to(dev)
    return net, x, labels


def lib_step(net, x, labels, classes):
    def step():
        net.zero_grad(set_to_none=True)
        lp, tf = net(x)
        loss = F.nll_loss(lp.reshape(-1, classes), labels.reshape(-1)) + 0.001 * M.feature_transform_reguliarzer(tf)
        loss.backward()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=0, help=argparse.SUPPRESS)   # (the child of the rocprofv3 run)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    net, x, labels = seg_setup(dev)
    if args.profile_steps:
        step = lib_step(net, x, labels, 13)
        for _ in range(args.profile_steps):
            step()
        torch.cuda.synchronize()
        return
    res = {"metric": "pointnet_v1", "device": torch.cuda.get_device_name(0)}
    res["seg_step_ms"] = round(timeit(lib_step(net, x, labels, 13), args.reps), 3)

    P = V.Params(net.state_dict(), torch.float32, dev)

    def torch_step():
        for v in P.p.values():
            v.grad = None
        lp, _, tf = V.seg_forward(P, x, True, True, "concat")
        V.train_loss(lp, labels, tf).backward()
    res["seg_step_torch_ms"] = round(timeit(torch_step, args.reps), 3)
    del P

    torch.manual_seed(0)
    enet = M.PointNetSeg(19, 4, True).to(dev).eval()
    cloud = torch.randn(1, 4, 25000, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)

    def infer():
        with torch.no_grad():
            enet(cloud)
    res["seg_eval_ms"] = round(timeit(infer, args.reps), 3)

    torch.manual_seed(0)
    cnet = M.PointNetCls(40, True).to(dev).train()
    for m in cnet.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    gen = torch.Generator(device="cpu").manual_seed(3)
    cx = torch.randn(16, 3, 1024, generator=gen).to(dev)
    cl = torch.randint(0, 40, (16,), generator=gen).to(dev)
    res["cls_step_ms"] = round(timeit(lib_step(cnet, cx, cl, 40), args.reps), 3)

    if not args.no_profile and shutil.which("rocprofv3"):
        res["top_kernels"] = profile(args)
    print(json.dumps(res))


def profile(args, steps=10, top=12):
    """One rocprofv3 --kernel-trace --stats run of `steps` library Seg steps in a child process: [(kernel, total us, calls)]."""
    d = tempfile.mkdtemp(prefix="pn1_prof_")
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
