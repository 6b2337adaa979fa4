#!/usr/bin/env python3
"""The reference's part-segmentation loop (partseg.py) on synthetic shapes, every step of it on the HIP library: resident
``[M, 6]`` shapes (``shapes.ShapeStore``) -> pn2_prepare_shapes (rotate, jitter, resample; draws on the device) ->
PointNet2PartSegMsg_one_hot(50) forward -> nll_loss -> backward -> pn2_adam_step (``--optimizer SGD``: partseg.py:113's
SGD(lr=0.01, momentum=0.9) -> pn2_sgd_step).

The part label of a point is a function of its category and its height inside the normalised shape, so the loss must fall; the
script prints the loss curve and the all-inclusive time per step (batch preparation + step + optimiser).

    python tools/train_partseg.py --steps 20 --batch 16 --npoints 2048 [--optimizer SGD]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointnet12_amd import optim, parallel, pointnet2, shapes     # noqa: E402
from pointnet12_amd.loss import nll_loss                          # noqa: E402

PARTS, CATEGORIES = 50, 16


def synthetic_shapes(count, M, seed=0):
    """``count`` ellipsoid-ish shapes of about M points: (normalised xyz, outward normals), 3 height bands of parts per category."""
    rng = np.random.default_rng(seed)
    clouds, segs, cats = [], [], []
    for i in range(count):
        m = int(M * rng.uniform(0.9, 1.1))
        cat = i % CATEGORIES
        d = rng.normal(size=(m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        axes = np.array([1.0, 0.4 + 0.04 * cat, 0.3 + 0.02 * cat])
        xyz = shapes.point_cloud_normalize((d * axes * rng.uniform(0.6, 1.0, (m, 1))).astype(np.float32))
        nrm = d / axes
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        band = np.clip(((xyz[:, 1] + 0.5) * 3).astype(np.int64), 0, 2)
        clouds.append(np.concatenate([xyz, nrm], 1).astype(np.float32))
        segs.append((cat * 3 + band).astype(np.int32))               # 48 of the 50 part labels
        cats.append(cat)
    return clouds, segs, cats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--shapes", type=int, default=64)
    ap.add_argument("--raw-points", type=int, default=2700)
    ap.add_argument("--lr", type=float, default=1e-3, help="Adam's learning rate (SGD takes the reference's 0.01)")
    ap.add_argument("--optimizer", choices=("Adam", "SGD"), default="Adam")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    store = shapes.ShapeStore(*synthetic_shapes(args.shapes, args.raw_points), device=dev)
    net = pointnet2.PointNet2PartSegMsg_one_hot(PARTS).to(dev)
    net.train()
    bucket = parallel.FlatGradBucket(net, direct=True)
    if args.optimizer == "SGD":
        opt = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, bucket=bucket, fused_zero_grad=True)
    else:
        opt = optim.Adam(net.parameters(), lr=args.lr, betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4, bucket=bucket,
                         fused_zero_grad=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    pick = np.random.default_rng(0)
    out = (torch.empty(args.batch, args.npoints, 6, device=dev), torch.empty(args.batch, args.npoints, device=dev, dtype=torch.int64),
           torch.empty(args.batch, device=dev, dtype=torch.int64))
    curve = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.steps):
        pts, seg, cls = shapes.prepare_shapes(store, pick.integers(0, len(store), args.batch), args.npoints, rotate=True,
                                              jitter=True, rng=gen, out=out)
        one_hot = torch.nn.functional.one_hot(cls, CATEGORIES).float()                 # to_categorical of partseg.py
        opt.zero_grad()                                            # free after the first step (fused into the optimiser's)
        lp = net(pts[..., 0:3].transpose(2, 1), pts[..., 3:6].transpose(2, 1), one_hot)
        loss = nll_loss(lp.reshape(-1, PARTS), seg.reshape(-1))
        loss.backward()
        bucket.all_reduce()
        opt.step()
        if it % max(args.steps // 20, 1) == 0 or it == args.steps - 1:
            curve.append((it, round(float(loss.detach()), 4)))     # the float() is this loop's only sync
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"net": "partseg_msg_one_hot", **({"optimizer": "SGD"} if args.optimizer == "SGD" else {}), "steps": args.steps, "batch": args.batch, "npoints": args.npoints,
                      "ms_per_step_all_in": round(dt / args.steps * 1e3, 3), "loss_first": curve[0][1], "loss_last": curve[-1][1],
                      "curve": curve}))


if __name__ == "__main__":
    main()
