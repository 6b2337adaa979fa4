#!/usr/bin/env python3
"""Batch preparation on the HIP library (pointnet12_amd/shapes.py) against the reference's formulation in the same run: the
per-item numpy ``__getitem__`` loop of a ``num_workers=0`` DataLoader, collate, ``.cuda()``, on one GPU.

    python tools/bench_shapes.py [--reps 20]

Prints one JSON line.  Per workload, every batch with augmentation on:

  shapenet  32 x 2048 x (3 + 3) out of 64 shapes of ~2 700 points   PartNormalDataset.__getitem__ (ShapeNetDataLoader.py:95-127)
  modelnet  32 x 2048 x 3 out of 64 items                           ModelNetDataLoader.__getitem__ as it is meant (:60-70)
  s3dis     16 x 4096 x 9 out of 32 blocks                          S3DISDataLoader.__getitem__ (s3dis.S3DISDataLoader)

  host_ms       the reference's formulation: numpy items, np.stack, torch.from_numpy(...).cuda(); host clock to the end of the copy
  numpy_rng_ms  prepare_shapes(rng="numpy"): the same numpy draws (bit-equal batches), the rest on the device
  device_rng_ms prepare_shapes(rng=torch.Generator): the draws on the device too
  call_us       prepare_shapes on resident draws (a Draws tuple) into preallocated buffers: device events around one eager call on
                an idle device, so the launch latency is inside it
  replay_us     the same call captured 32 times into one graph: replay time / 32 (device events), the cost inside a captured step
  equal         host and rng="numpy" gave the same bits under the same seed

Medians of --reps after warm-up; the ways alternate inside every repetition.  Nothing is asserted.
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

from pointnet12_amd import shapes as S                # noqa: E402


def host_ms(fns, reps, warmup=3):
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


# ------------------------------------------------------------------------------------------------ the formulation being replaced
def host_shapenet_item(rows, seg, npoints):
    pointcloud, normal = rows[:, 0:3], rows[:, 3:6]                # (normalised at fill time in both ways)
    pointcloud = np.expand_dims(pointcloud, axis=0)
    pointcloud = S.rotate_point_cloud(pointcloud)
    pointcloud = S.jitter_point_cloud(pointcloud).astype(np.float32)
    pointcloud = np.squeeze(pointcloud, axis=0)
    choice = np.random.choice(len(seg), npoints, replace=True)
    return pointcloud[choice, :], seg[choice], normal[choice, :]


def host_modelnet_item(cloud):
    pcd = np.expand_dims(cloud, axis=0)
    pcd = S.rotate_point_cloud(pcd)
    pcd = S.jitter_point_cloud(pcd).astype(np.float32)
    return np.squeeze(pcd, axis=0)


def host_s3dis_item(block):
    return (block + np.clip(0.01 * np.random.randn(*block.shape), -0.05, 0.05)).astype(np.float32)


def collate(arrays, dev):
    return torch.from_numpy(np.stack(arrays)).to(dev)


def workload(kind, reps, dev):
    rng = np.random.default_rng(17)
    res = {}
    if kind == "shapenet":
        B, N, C, nc, rot, npoints = 32, 2048, 6, 3, True, 2048
        clouds = [rng.uniform(-1, 1, (int(m), 6)).astype(np.float32) for m in rng.integers(2500, 2900, 64)]
        labels = [rng.integers(0, 50, len(c)).astype(np.int32) for c in clouds]

        def host(ids):
            items = [host_shapenet_item(clouds[i], labels[i], N) for i in ids]
            return (torch.cat([collate([it[0] for it in items], dev), collate([it[2] for it in items], dev)], 2),
                    collate([it[1] for it in items], dev).long())
    elif kind == "modelnet":
        B, N, C, nc, rot, npoints = 32, 2048, 3, 3, True, None
        clouds = rng.uniform(-1, 1, (64, 2048, 3)).astype(np.float32)
        labels = None

        def host(ids):
            return collate([host_modelnet_item(clouds[i]) for i in ids], dev), None
    else:
        B, N, C, nc, rot, npoints = 16, 4096, 9, 9, False, None
        clouds = rng.uniform(0, 1, (32, 4096, 9)).astype(np.float32)
        labels = rng.integers(0, 13, (32, 4096)).astype(np.uint8)

        def host(ids):
            return collate([host_s3dis_item(clouds[i]) for i in ids], dev), collate([labels[i] for i in ids], dev).long()
    store = S.ShapeStore(clouds, labels, None, dev)
    ids = rng.integers(0, len(store), B)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def way_host():
        np.random.seed(5)
        res["host"] = host(ids)

    def way_numpy():
        np.random.seed(5)
        res["numpy"] = S.prepare_shapes(store, ids, npoints, rotate=rot, jitter=True, noise_cols=nc)[:2]

    def way_device():
        S.prepare_shapes(store, ids, npoints, rotate=rot, jitter=True, noise_cols=nc, rng=gen)

    host_t, numpy_t, device_t = host_ms([way_host, way_numpy, way_device], reps)
    d = S.draw(store, ids, npoints, rotate=rot, jitter=True, noise_cols=nc, rng=gen)
    out = (torch.empty(B, N, C, device=dev), torch.empty(B, N, dtype=torch.int64, device=dev) if labels is not None else None, None)
    call = event_ms(lambda: S.prepare_shapes(store, None, N, rng=d, out=out), reps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for _ in range(32):
                S.prepare_shapes(store, None, N, rng=d, out=out)
    torch.cuda.current_stream().wait_stream(side)
    replay = event_ms(graph.replay, reps) / 32
    equal = torch.equal(res["host"][0].view(torch.int32), res["numpy"][0].view(torch.int32)) and \
        (res["host"][1] is None or torch.equal(res["host"][1], res["numpy"][1]))
    return {"shape": "%dx%dx%d" % (B, N, C), "host_ms": round(host_t, 3), "numpy_rng_ms": round(numpy_t, 3),
            "device_rng_ms": round(device_t, 3), "call_us": round(call * 1e3, 2), "replay_us": round(replay * 1e3, 2),
            "speedup_numpy_rng": round(host_t / numpy_t, 2), "speedup_device_rng": round(host_t / device_t, 2), "equal": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "prepare_shapes", "device": torch.cuda.get_device_name(0), "reps": args.reps, "workloads": {}}
    for kind in ("shapenet", "modelnet", "s3dis"):
        res["workloads"][kind] = workload(kind, args.reps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
