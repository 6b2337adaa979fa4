#!/usr/bin/env python3
"""Device time of the section-8(f)3 kernels at benchmark sizes (HIP events on the launch stream): pn2_adam_step,
pn2_sgd_step (against torch.optim.SGD over the tensors of PointNet2SemSegMsg, eager and as a captured launch) and
pn2_prepare_clouds.

    python tools/bench_train.py            # one JSON line per kernel
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointnet12_amd import _lib, loader, optim      # noqa: E402


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us


def median_us(fn, reps=20, inner=10, warm=3):
    """Median over ``reps`` samples of the time per call, each sample ``inner`` back-to-back calls between one pair of events (a
    single call between two events times the launch latency, which a training step hides behind the work queued before it)."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner * 1e3)
    return float(np.median(out))


def captured(opt):
    """``opt.step()`` as one hipGraph; returns its replay."""
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.synchronize()
    return graph.replay


def sgd_leg(dev):
    """optim.SGD against torch.optim.SGD (momentum 0.9, the reference's branch) over the parameter tensors of PointNet2SemSegMsg:
    one launch over the flat buffer against foreach launches over the tensor list, eager and captured.  (A captured
    torch.optim.SGD.step() holds the lr of the capture; it is timed here, not recommended.)"""
    from pointnet12_amd import pointnet2
    shapes = [tuple(p.shape) for p in pointnet2.PointNet2SemSegMsg(13, feature_dims=1).parameters()]
    n = sum(int(np.prod(s)) for s in shapes)

    def params():
        return [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]

    res = {"kernel": "pn2_sgd_step", "case": "msg_semseg", "tensors": len(shapes), "elements": n}
    for mode in ("eager", "graph"):
        mine_p, ref_p = params(), params()
        mine = optim.SGD(mine_p, lr=0.01, momentum=0.9, device_step=mode == "graph")
        ref = torch.optim.SGD(ref_p, lr=0.01, momentum=0.9)
        for p, q in zip(mine_p, ref_p):
            p.grad.normal_()
            q.grad = torch.randn_like(q)
        mine.step()                                            # past the first step: the buffer is read from here on
        ref.step()
        torch.cuda.synchronize()
        us = median_us(mine.step if mode == "eager" else captured(mine))
        us_ref = median_us(ref.step if mode == "eager" else captured(ref))
        if mode == "eager":                                    # the launch's own device time, and its rate over 20 B/element:
            with _lib.call_profile() as calls:                 # p, g, buf read, p, buf written (no fused zero-grad here)
                for _ in range(20):
                    mine.step()
                torch.cuda.synchronize()
            ker = float(np.median([a.elapsed_time(b) for _, _, a, b, _k in calls])) * 1e3
            res["kernel_us"], res["kernel_GB/s"] = round(ker, 2), round(20.0 * n / ker / 1e3, 1)
        res["%s_us" % mode] = round(us, 2)
        res["torch_%s_us" % mode] = round(us_ref, 2)
    print(json.dumps(res))


def main():
    dev = torch.device("cuda:0")
    _lib.load()
    for name, n in (("ssg_semseg", 968173), ("msg_semseg", 1735001), ("x16", 16 * 1735001)):
        p = [torch.nn.Parameter(torch.randn(n, device=dev))]
        opt = optim.Adam(p, lr=1e-3, weight_decay=1e-4)
        p[0].grad.normal_()
        us = timed(opt.step)
        ref_p = [torch.nn.Parameter(torch.randn(n, device=dev))]
        ref = torch.optim.Adam(ref_p, lr=1e-3, weight_decay=1e-4)
        ref_p[0].grad = torch.randn(n, device=dev)
        us_ref = timed(ref.step)
        print(json.dumps({"kernel": "pn2_adam_step", "case": name, "elements": n, "us": round(us, 2),
                          "GB/s": round(28.0 * n / us / 1e3, 1), "aten_single_tensor_us": round(us_ref, 2)}))
    sgd_leg(dev)
    rng = np.random.default_rng(0)
    for B, M, N in ((16, 20000, 4096), (8, 120000, 65536)):
        scans = [rng.uniform(-60, 60, (M, 4)).astype(np.float32) for _ in range(B)]
        labels = [rng.integers(0, 19, M).astype(np.int32) for _ in range(B)]
        store = loader.ScanStore(scans, labels, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        whole = timed(lambda: loader.prepare_batch(store, list(range(B)), N, train=True, rng=gen), reps=20)
        with _lib.call_profile() as calls:
            for _ in range(20):
                loader.prepare_batch(store, list(range(B)), N, train=True, rng=gen)
            torch.cuda.synchronize()
        ker = float(np.median([a.elapsed_time(b) for _, _, a, b, _k in calls])) * 1e3
        # algorithmic bytes per output point: choice 8 + raw row 16 + noise row 16 + label 4 + out 16 + label out 8
        print(json.dumps({"kernel": "pn2_prepare_clouds", "B": B, "M": M, "N": N, "kernel_us": round(ker, 2),
                          "GB/s": round(68.0 * B * N / ker / 1e3, 1), "prepare_batch_device_rng_us": round(whole, 1)}))


if __name__ == "__main__":
    main()
