#!/usr/bin/env python3
"""Segmentation metrics on the HIP library (pointnet12_amd/metrics.py) against the reference's formulation in stock PyTorch on the
same device (the class loop with its blocking reads, the per-cloud numpy passes), on one GPU.

    python tools/bench_metrics.py [--reps 20] [--pass-batches 20] [--no-pass]

Prints one JSON line.  Per workload, each on a fixed log_probs / target already on the device:

  semseg  16 x 4096 x 13        calc_categorical_iou + the accuracy read of test_semseg (pcd_utils.py:193-200)
  kitti   4 x 100000 x 20       the class loop and accuracy read of test_kitti_semseg (pcdseg.py:75-86)
  partseg 16 x 2048 x 50        compute_cat_iou + the accuracy read of test_partseg (pcd_utils.py:155-162), per cloud

  stock_ms      the reference's formulation, host clock around the call (it ends in blocking reads); median of --reps
  new_ms        this package's function of the same name / the same statistics from ONE table read (host clock, one read-back)
  update_ms     what a batch costs inside an evaluation loop: SegEvaluator.update, host clock to the end of the device work
  kernel_us     pn2_seg_confusion alone into a preallocated table (device events)
  kernel_gbps   (4 C + 8) bytes per row (the class columns and the label) over kernel time; roofline_fraction against 8 TB/s
  equal         the two ways returned the same numbers (bitwise)

and, unless --no-pass, one whole test_semseg pass of --pass-batches batches of 16 x 4096 on an eval-mode PointNet2SemSeg both
ways (pass_new_ms, pass_stock_ms: host clock, median of --reps/4 passes).  Runs of the two ways alternate inside every repetition.
"""
import argparse
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                          # noqa: E402

from pointnet12_amd import metrics as M               # noqa: E402

ROOFLINE_BYTES_PER_S = 8e12


# ------------------------------------------------------------------------------------------------ the formulation being replaced
def stock_calc_categorical_iou(pred, target, num_classes, iou_tabel):
    choice = pred.max(2)[1]
    for cat in range(num_classes):
        I = torch.sum((choice == cat) & (target == cat)).float()
        U = torch.sum((choice == cat) | (target == cat)).float()
        iou = 1 if U == 0 else (I / U).cpu().numpy()
        iou_tabel[cat, 0] += iou
        iou_tabel[cat, 1] += 1
    return iou_tabel


def stock_accuracy(pred, target, num_classes):
    choice = pred.contiguous().view(-1, num_classes).max(1)[1]
    return choice.eq(target.view(-1, 1)[:, 0]).cpu().sum().item() / target.numel()


def stock_compute_cat_iou(pred, target, num_classes, iou_tabel):
    iou_list = []
    target = target.cpu().numpy()
    for j in range(pred.size(0)):
        choice = pred[j].max(1)[1].cpu().numpy()
        for cat in range(num_classes):
            I = np.sum(np.logical_and(choice == cat, target[j] == cat))
            U = np.sum(np.logical_or(choice == cat, target[j] == cat))
            iou = 1 if U == 0 else I / float(U)
            iou_tabel[cat, 0] += iou
            iou_tabel[cat, 1] += 1
            iou_list.append(iou)
    return iou_tabel, iou_list


def stock_kitti_batch(pred, target, num_classes, ious, count):
    choice = pred.argmax(-1)
    for class_id in range(num_classes):
        I = torch.sum((choice == class_id) & (target == class_id)).cpu().item()
        U = torch.sum((choice == class_id) | (target == class_id)).cpu().item()
        ious[class_id] += 1 if U == 0 else I / U
        count[class_id] += 1
    return (choice == target).sum().cpu().item() / target.numel()


def stock_test_semseg(model, loader, catdict, num_classes):
    iou_tabel = np.zeros((len(catdict), 3))
    metrics = defaultdict(list)
    with torch.no_grad():
        for points, target in loader:
            points, target = points.float().transpose(2, 1).cuda(), target.long().cuda()
            pred = model(points)
            iou_tabel = stock_calc_categorical_iou(pred, target, num_classes, iou_tabel)
            metrics["accuracy"].append(stock_accuracy(pred, target, num_classes))
    iou_tabel[:, 2] = iou_tabel[:, 0] / iou_tabel[:, 1]
    return {"accuracy": np.mean(metrics["accuracy"]), "iou": np.mean(iou_tabel[:, 2])}


# ------------------------------------------------------------------------------------------------ timing
def host_ms(fns, reps, warmup=3):
    """Median host time of each callable to the end of its device work, the callables taken in turn inside every repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in times]


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        out.append(a.elapsed_time(e))
    return float(np.median(out))


def inputs(B, N, C, dev):
    gen = torch.Generator().manual_seed(B + N + C)
    target = torch.randint(0, C, (B, (N + 31) // 32), generator=gen).repeat_interleave(32, dim=1)[:, :N].contiguous()
    logits = torch.randn(B, N, C, generator=gen)
    logits.scatter_add_(2, target[:, :, None], torch.full((B, N, 1), 2.0))
    return torch.log_softmax(logits, -1).to(dev), target.to(dev)


def bench_workload(kind, B, N, C, reps, dev):
    lp, tg = inputs(B, N, C, dev)
    results = {}

    if kind == "semseg":
        def stock():
            results["stock"] = (stock_calc_categorical_iou(lp, tg, C, np.zeros((C, 3))), stock_accuracy(lp, tg, C))

        def new():
            table = M.confusion(lp, tg, C).cpu().numpy()
            results["new"] = (M._add_categorical_iou(table, C, np.zeros((C, 3))), M._correct(table) / tg.numel())
    elif kind == "kitti":
        def stock():
            ious, count = np.zeros(C, np.float32), np.zeros(C, np.uint32)
            results["stock"] = (stock_kitti_batch(lp, tg, C, ious, count), ious)

        def new():
            table = M.confusion(lp, tg, C).cpu().numpy()
            inter, union = M.iou_counts(table)
            ious = np.zeros(C, np.float32)
            for c in range(C):
                ious[c] += 1 if union[c] == 0 else int(inter[c]) / int(union[c])
            results["new"] = (M._correct(table) / tg.numel(), ious)
    else:
        def stock():
            results["stock"] = (stock_compute_cat_iou(lp, tg, C, np.zeros((C, 3))), stock_accuracy(lp, tg, C))

        def new():
            tables = M.confusion(lp, tg, C, per_cloud=True).cpu().numpy()
            results["new"] = (M._add_cat_iou(tables, C, np.zeros((C, 3)), []), M._correct(tables) / tg.numel())

    per_cloud = kind == "partseg"
    tape = [M.SegEvaluator(C, per_cloud=per_cloud)]

    def update():
        if len(tape[0]) > 4096:                              # (an evaluation pass of a few hundred batches; then a fresh tape)
            tape[0] = M.SegEvaluator(C, per_cloud=per_cloud)
        tape[0].update(lp, tg)

    out = torch.zeros((B, C + 1, C) if per_cloud else (C + 1, C), device=dev, dtype=torch.int64)
    stock_ms, new_ms, update_ms = host_ms([stock, new, update], reps)
    kernel_ms = event_ms(lambda: M.confusion(lp, tg, C, per_cloud=per_cloud, out=out), reps)
    nbytes = float(B) * N * (4 * C + 8)

    def flat(x):
        if isinstance(x, (tuple, list)):
            return [v for y in x for v in flat(y)]
        return [np.asarray(x, np.float64).tobytes()]
    return {"shape": "%dx%dx%d" % (B, N, C), "stock_ms": round(stock_ms, 4), "new_ms": round(new_ms, 4), "update_ms": round(update_ms, 4),
            "kernel_us": round(kernel_ms * 1e3, 2), "kernel_gbps": round(nbytes / (kernel_ms * 1e-3) / 1e9, 1),
            "roofline_fraction": round(nbytes / (kernel_ms * 1e-3) / ROOFLINE_BYTES_PER_S, 4),
            "speedup": round(stock_ms / new_ms, 2), "equal": flat(results["stock"]) == flat(results["new"])}


def bench_pass(batches, reps, dev):
    from pointnet12_amd import pointnet2 as P
    from pointnet12_amd import synthetic as syn
    torch.manual_seed(0)
    net = P.PointNet2SemSeg(13, 6).to(dev).eval()
    distinct = [syn.kitti_batch(16 * i, 16, 4096) for i in range(2)]
    loader = [(torch.from_numpy(distinct[i % 2][0]).transpose(2, 1), torch.from_numpy(distinct[i % 2][1])) for i in range(batches)]
    catdict = {i: "class%02d" % i for i in range(13)}
    res = {}

    def new():
        metrics, _ = M.test_semseg(net, loader, catdict, "pointnet2", 13)
        res["new"] = (metrics["accuracy"], metrics["iou"])

    def stock():
        metrics = stock_test_semseg(net, loader, catdict, 13)
        res["stock"] = (metrics["accuracy"], metrics["iou"])

    stock_ms, new_ms = host_ms([stock, new], max(3, reps // 4), warmup=1)
    return {"batches": batches, "batch": "16x4096", "pass_stock_ms": round(stock_ms, 2), "pass_new_ms": round(new_ms, 2),
            "speedup": round(stock_ms / new_ms, 3), "equal": [float(v).hex() for v in res["new"]] == [float(v).hex() for v in res["stock"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pass-batches", type=int, default=20)
    ap.add_argument("--no-pass", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "seg_metrics", "device": torch.cuda.get_device_name(0), "reps": args.reps, "workloads": {}}
    for kind, B, N, C in (("semseg", 16, 4096, 13), ("kitti", 4, 100000, 20), ("partseg", 16, 2048, 50)):
        res["workloads"][kind] = bench_workload(kind, B, N, C, args.reps, dev)
    if not args.no_pass:
        res["test_semseg_pass"] = bench_pass(args.pass_batches, args.reps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
