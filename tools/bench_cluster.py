#!/usr/bin/env python3
"""Euclidean clustering on the HIP library (``pn2_voxel_components`` through ``voxel.VoxelGrid.components``) against the host
formulation on the same cells, in the same run.

    python tools/bench_cluster.py [--reps 20] [--host-reps 5] [--seed 0] [--only scan,scans16,clouds,snake]

Prints one JSON line.  The three workloads of tools/bench_voxel.py (``scan``: 120 000 rows of a scanner model at 0.1 m, ``scans16``: 16
of them in one call, ``clouds``: 16 x 4 096 normalised rows at 0.02) and ``snake``: a one-cell-wide serpentine path of 20 000 voxels,
rows in ascending order -- under connectivity 6 every voxel links to its predecessor, the deepest forest the union can be asked for.
Each is gridded ONCE (``downsample``, not timed) and then clustered at connectivity 6, 18 and 26:

  eager_ms  ``components(out=...)`` into preallocated buffers: every output (row and voxel ids, the four per-component arrays, the count)
  graph_ms  the same call captured into a graph, replayed
  host_ms   the host formulation on the same cells, already in host memory: the occupied cells packed into sorted int64 keys, one
            ``np.searchsorted`` per half-neighbour offset for the edge list, ``scipy.sparse.csgraph.connected_components`` on it (where
            scipy imports; else the dict-and-union-find restatement of tests/cluster_ref.py, ``host`` says which), per cloud.  It
            returns labels in scipy's order, not numbered by root, and no per-row map; it is timed as it is
  components, same_count   the number of components, which must be the same on both sides

Device times are medians of --reps runs after 3 warm-up runs, the host's of --host-reps runs, host clock around the device work (a
synchronize on either side).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch                                          # noqa: E402

from bench_voxel import scanner_scan, timed_ms        # noqa: E402
from pointnet12_amd import synthetic, voxel           # noqa: E402

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    HOST = "scipy.sparse.csgraph.connected_components"
except ImportError:                                   # pragma: no cover
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cluster_ref
    HOST = "tests/cluster_ref.py"

HALF = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1), (1, -1, 1),
        (1, -1, -1)]
TAKE = {6: 3, 18: 9, 26: 13}


def snake_rows(n, width=25):
    """Rows in the middle of the cells of a serpentine path in the plane z = 0 (``voxel = 1``), in path order."""
    cells, x, y, step = [], 0, 0, 1
    while len(cells) < n:
        for _ in range(width):
            cells.append((x, y, 0))
            x += step
        x -= step
        cells.append((x, y + 1, 0))
        y += 2
        step = -step
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = np.array(cells[:n], np.float32) + 0.5
    return pts


def host_components(cells, connectivity):
    """The number of components of one cloud's cells (int64 ``[V, 3]``, all within +-2^19)."""
    if HOST.startswith("tests"):
        return cluster_ref.components_of_cells(cells, np.ones(len(cells), np.int64), connectivity=connectivity)["count"]
    V = len(cells)
    if V == 0:
        return 0
    pack = lambda c: ((c[:, 0] + (1 << 20)) << 42) | ((c[:, 1] + (1 << 20)) << 21) | (c[:, 2] + (1 << 20))
    key = pack(cells)
    order = np.argsort(key)
    sorted_key = key[order]
    src, dst = [], []
    for d in HALF[:TAKE[connectivity]]:
        want = pack(cells + np.array(d, np.int64))
        at = np.minimum(np.searchsorted(sorted_key, want), V - 1)
        hit = sorted_key[at] == want
        src.append(np.flatnonzero(hit))
        dst.append(order[at[hit]])
    src, dst = np.concatenate(src), np.concatenate(dst)
    graph = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(V, V)).tocsr()
    return int(connected_components(graph, directed=False)[0])


def workload(name, B, M, size, reps, host_reps, dev, rng):
    if name == "clouds":
        pts = np.concatenate([synthetic.kitti_cloud(int(rng.integers(1 << 30)), M)[:, :4] for _ in range(B)], 0)
    elif name == "snake":
        pts = snake_rows(M)
    else:
        pts = np.concatenate([scanner_scan(rng, M) for _ in range(B)], 0)
    points = torch.from_numpy(pts).to(dev)
    begin = torch.arange(B, device=dev, dtype=torch.int64) * M
    count = torch.full((B,), M, device=dev, dtype=torch.int64)
    vg = voxel.VoxelGrid(size, device=dev)
    down = vg.downsample(points, None, begin, count, M, out=vg.buffers(B * M, B, M))
    vg.check()
    voxels = down[3].cpu().tolist()
    # the same cells on the host: the representatives' rows, the rule's fp64 floor
    cells = [np.floor(down[0][b * M:b * M + voxels[b], :3].cpu().numpy().astype(np.float64) / size).astype(np.int64) for b in range(B)]
    res = {"B": B, "rows": M, "voxel": size, "voxels": int(sum(voxels))}
    cbufs = vg.component_buffers(B * M, B, M)
    for connectivity in (6, 18, 26):
        eager = lambda: vg.components(points, down, connectivity=connectivity, row_begin=begin, row_count=count, max_rows=M, out=cbufs)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eager()
        runs = {"eager_ms": eager, "graph_ms": graph.replay}
        for fn in runs.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():
                times[k].append(timed_ms(fn))
        one = {k: round(float(np.median(v)), 4) for k, v in times.items()}
        host_times, host_count = [], 0
        for _ in range(host_reps):
            t0 = time.perf_counter()
            host_count = sum(host_components(c, connectivity) for c in cells)
            host_times.append((time.perf_counter() - t0) * 1e3)
        one["host_ms"] = round(float(np.median(host_times)), 4)
        eager()
        vg.check()
        one["components"] = int(cbufs.count.sum().item())
        one["same_count"] = one["components"] == host_count
        res[str(connectivity)] = one
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="scan,scans16,clouds,snake")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cluster.py needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda")
    rng = np.random.default_rng(args.seed)
    shapes = {"scan": (1, 120000, 0.1), "scans16": (16, 120000, 0.1), "clouds": (16, 4096, 0.02), "snake": (1, 20000, 1.0)}
    out = {"reps": args.reps, "host_reps": args.host_reps, "host": HOST, "device": torch.cuda.get_device_name(0)}
    for name in args.only.split(","):
        out[name] = workload(name, *shapes[name], args.reps, args.host_reps, dev, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
