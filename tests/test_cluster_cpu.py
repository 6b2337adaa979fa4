"""CPU: the Euclidean-clustering rule (include/pn2.h, ``pn2_voxel_components``) as tests/cluster_ref.py states it, held to a brute-force
flood fill written here and, where scipy imports, to ``scipy.ndimage.label`` on dense lattices; ``kitti.write_labels(...,
instances=)``; the entry point's argument checks (no launch, no GPU) and the "no scratch" check of csrc/voxel_cluster.hip."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref as R
from conftest import ROOT
from pointnet12_amd import _lib, kitti


def flood_fill(cells, part, labels, connectivity, same_label):
    """Brute force over all pairs: every voxel takes the lowest id among itself and its neighbours until nothing changes.  Returns
    the lowest member of every voxel's component (-1: takes no part)."""
    cells = np.asarray(cells).astype(np.int64)
    V = len(cells)
    d = cells[:, None, :] - cells[None, :, :]
    differing = (d != 0).sum(2)
    near = (np.abs(d).max(2) <= 1) & (differing > 0) & (differing <= {6: 1, 18: 2, 26: 3}[connectivity])
    near &= part[:, None] & part[None, :]
    if same_label and labels is not None:
        near &= np.asarray(labels)[:, None] == np.asarray(labels)[None, :]
    comp = np.where(part, np.arange(V), -1)
    while True:
        best = comp.copy()
        for v in np.flatnonzero(part):
            best[v] = min(comp[v], comp[near[v]].min(initial=V))
        if np.array_equal(best, comp):
            return comp
        comp = best


def random_cells(rng, V, side):
    """V distinct cells of a side^3 lattice that straddles the origin, in random order."""
    flat = rng.choice(side ** 3, V, replace=False)
    return np.stack([flat % side, (flat // side) % side, flat // (side * side)], 1) - side // 2


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("seed,V,side,labelled,same_label", [(0, 150, 8, False, True), (1, 200, 7, True, True), (2, 200, 7, True, False),
                                                             (3, 1, 3, True, True), (4, 60, 30, False, True)])
def test_restatement_against_flood_fill(connectivity, seed, V, side, labelled, same_label):
    rng = np.random.default_rng(seed)
    cells = random_cells(rng, V, side)
    n_points = rng.integers(1, 6, V)
    labels = rng.integers(-1, 4, V).astype(np.int32) if labelled else None          # -1: takes no part; 3: beyond member
    member = np.array([1, 0, 1], np.int32) if labelled else None
    ref = R.components_of_cells(cells, n_points, labels, connectivity, same_label, member, min_points=4, min_voxels=2)
    part = R.takes_part(labels, member, V)
    if labelled and V > 10:
        assert part.any() and not part.all() and np.array_equal(part, np.isin(labels, (0, 2)))
    lowest = flood_fill(cells, part, labels, connectivity, same_label)
    assert np.array_equal(ref["part_root"], lowest)
    # the kept components by hand: numbered in ascending order of the lowest member
    ids, roots = np.full(V, -1), []
    for r in sorted(set(lowest[lowest >= 0].tolist())):
        mine = lowest == r
        if n_points[mine].sum() >= 4 and mine.sum() >= 2:
            ids[mine] = len(roots)
            roots.append(r)
    assert np.array_equal(ref["vox_component"], ids) and ref["count"] == len(roots) and ref["root"].tolist() == roots
    assert ref["points"].tolist() == [int(n_points[lowest == r].sum()) for r in roots]
    assert ref["voxels"].tolist() == [int((lowest == r).sum()) for r in roots]
    assert ref["label"].tolist() == [int(labels[r]) if labelled else 0 for r in roots]


@pytest.mark.parametrize("connectivity,density", [(6, 0.33), (18, 0.15), (26, 0.11), (26, 0.5)])
def test_restatement_against_scipy_on_dense_lattices(connectivity, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(connectivity)
    side = 14
    occupied = rng.random((side, side, side)) < density
    cells = np.argwhere(occupied)
    cells = cells[rng.permutation(len(cells))] - 5
    ref = R.components_of_cells(cells, np.ones(len(cells), np.int64), connectivity=connectivity)
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    lab, n = ndimage.label(occupied, structure)
    theirs = lab[tuple((cells + 5).T)]
    assert ref["count"] == n and (n > 3 or density == 0.5)                # (half full: one component)
    # the same partition: their label <-> our id is a bijection; our ids ascend with the lowest member
    pairs = set(zip(theirs.tolist(), ref["vox_component"].tolist()))
    assert len(pairs) == n
    first = [int(np.flatnonzero(ref["vox_component"] == i)[0]) for i in range(n)]
    assert first == sorted(first) and ref["root"].tolist() == first
    assert np.array_equal(ref["voxels"], np.bincount(ref["vox_component"]))


def test_axis_ends_and_diagonals():
    top, low = (1 << 20) - 1, -(1 << 20)
    for c in (6, 18, 26):
        # adjacent in the packed key, not in space
        assert R.components_of_cells([(0, 0, top), (0, 1, low)], [1, 1], connectivity=c)["count"] == 2
        assert R.components_of_cells([(0, top, 5), (1, low, 5)], [1, 1], connectivity=c)["count"] == 2
        assert R.components_of_cells([(0, 0, top - 1), (0, 0, top)], [1, 1], connectivity=c)["count"] == 1
        assert R.components_of_cells([(low, 3, 3), (low + 1, 3, 3)], [1, 1], connectivity=c)["count"] == 1
    cells = [(0, 0, 0), (1, 1, 0), (2, 2, 1), (5, 5, 5), (5, 5, 6)]    # an edge neighbour, then a corner neighbour, a face pair apart
    assert [R.components_of_cells(cells, [1] * 5, connectivity=c)["count"] for c in (6, 18, 26)] == [4, 3, 2]


def test_rows_rule_and_snake():
    cells = R.snake_cells(2000)
    assert len(np.unique(cells, axis=0)) == 2000 and (np.abs(np.diff(cells, axis=0)).sum(1) == 1).all()
    assert R.components_of_cells(cells, np.ones(2000), connectivity=6)["count"] == 1
    ref = R.components_of_cells(np.delete(cells, 777, 0), np.ones(1999), connectivity=6)
    assert ref["count"] == 2 and ref["root"].tolist() == [0, 777] and ref["voxels"].tolist() == [777, 1222]
    # a road point in a car's cell never carries the car's id
    vox_component, vox_labels = np.array([0, -1, 1], np.int32), np.array([4, 9, 4], np.int32)
    rows = R.rows_of(vox_component, [0, 0, -1, 2, 1, 2], vox_labels, [4, 9, 4, 4, 9, 7])
    assert rows.tolist() == [0, -1, -1, 1, -1, -1]
    assert R.rows_of(vox_component, [0, 0, -1, 2, 1, 2]).tolist() == [0, 0, -1, 1, -1, 1]


def test_write_labels_with_instances(tmp_path):
    rng = np.random.default_rng(0)
    labels = rng.integers(0, 260, 500).astype(np.int32)
    inst = rng.integers(0, 65536, 500).astype(np.int32)
    inst[:2] = (0, 65535)
    a, b, c = (os.path.join(tmp_path, n) for n in ("a.label", "b.label", "c.label"))
    kitti.write_labels(a, labels)
    assert np.array_equal(np.fromfile(a, np.uint8), labels.astype("<u4").view(np.uint8))      # today's bytes
    kitti.write_labels(b, labels, instances=None)
    kitti.write_labels(c, labels, np.zeros(500, np.int64))
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    kitti.write_labels(b, labels, inst)
    words = np.fromfile(b, "<u4")
    assert np.array_equal(words & 0xFFFF, labels) and np.array_equal(words >> 16, inst) and words.dtype.itemsize == 4
    assert np.array_equal(words, (inst.astype(np.uint32) << 16) | labels.astype(np.uint32))
    import torch
    kitti.write_labels(c, torch.from_numpy(labels), torch.from_numpy(inst).long())
    assert open(b, "rb").read() == open(c, "rb").read()
    for bad in (inst[:-1], np.where(np.arange(500) == 7, 65536, inst), np.where(np.arange(500) == 9, -1, inst), inst.astype(np.float32)):
        with pytest.raises(ValueError):
            kitti.write_labels(c, labels, bad)
    with pytest.raises(ValueError):
        kitti.write_labels(c, np.where(np.arange(500) == 3, 65536, labels), inst)
    kitti.write_labels(c, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert os.path.getsize(c) == 0


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    d3 = lambda *v: (ctypes.c_double * 3)(*v)
    org, vox = d3(0, 0, 0), d3(0.1, 0.1, 0.1)
    a = 4096                                                          # a non-null, aligned stand-in: a refused call touches nothing
    vp = lambda x: None if x is None else ctypes.c_void_p(x)
    names = ("pts", "row_begin", "row_count", "origin", "voxel", "out_begin", "out_count", "out_index", "n_points", "comp_begin",
             "comp_count", "workspace")

    def call(ld=4, B=1, max_rows=16, connectivity=26, member=None, L=0, min_points=1, min_voxels=1, vox_labels=None, row_labels=None,
             inverse=a, row_component=None, **kw):
        g = {n: a for n in names}
        g.update(origin=org, voxel=vox)
        g.update(kw)
        ptr = lambda n: g[n] if n in ("origin", "voxel") else vp(g[n])
        return lib.pn2_voxel_components(ptr("pts"), ld, ptr("row_begin"), ptr("row_count"), B, max_rows, ptr("origin"), ptr("voxel"),
                                        ptr("out_begin"), ptr("out_count"), ptr("out_index"), ptr("n_points"), vp(vox_labels), vp(inverse),
                                        vp(row_labels), connectivity, 1, vp(member), L, min_points, min_voxels, ptr("comp_begin"), None,
                                        vp(row_component), None, None, None, None, ptr("comp_count"), None, ptr("workspace"), None)
    EINVAL = -1
    for n in names:
        assert call(**{n: None}) == EINVAL, n
    for c in (0, 4, 7, 8, 27, -6, 124):
        assert call(connectivity=c) == EINVAL
    assert call(B=0) == EINVAL and call(B=65536) == EINVAL and call(ld=2) == EINVAL and call(ld=17) == EINVAL
    assert call(max_rows=-1) == EINVAL and call(max_rows=_lib.VOXEL_MAX_ROWS + 1) == EINVAL
    assert call(min_points=0) == EINVAL and call(min_voxels=0) == EINVAL and call(min_points=-3) == EINVAL
    assert call(member=a, L=4) == EINVAL and call(member=a, L=0, vox_labels=a) == EINVAL          # member needs labels and L >= 1
    assert call(row_labels=a) == EINVAL                                                          # row_labels need the voxels' labels
    assert call(row_component=a, inverse=None) == EINVAL
    assert call(voxel=d3(0.1, 0.0, 0.1)) == EINVAL and call(voxel=d3(float("nan"), 0.1, 0.1)) == EINVAL
    assert call(origin=d3(0, float("inf"), 0)) == EINVAL
    assert call(pts=a + 2) == EINVAL and call(workspace=a + 8) == EINVAL
    wb = lib.pn2_voxel_components_workspace_bytes
    assert wb(0, 16) == EINVAL and wb(1, -1) == EINVAL and wb(65536, 16) == EINVAL and wb(1, _lib.VOXEL_MAX_ROWS + 1) == EINVAL
    sizes = [wb(1, m) for m in (0, 1, 63, 1024, 1025, 4096, 120000, 1 << 22)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    for m in (1, 1000, 120000):                                       # a table of at least 2 * max_rows 16-byte slots, 25 bytes a voxel
        assert wb(1, m) >= 2 * m * 16 + 25 * m
    by_b = [wb(B, 5000) for B in (1, 2, 3, 16, 65535)]
    assert all(s > 0 and s % 16 == 0 for s in by_b) and by_b == sorted(set(by_b))
    bits = (_lib.VOXEL_ERR_RANGE, _lib.VOXEL_ERR_ROWS, _lib.SEGMENT_ERR_RANGE, _lib.SEGMENT_ERR_NONFINITE, _lib.CLUSTER_ERR_INDEX,
            _lib.CLUSTER_ERR_CELL, _lib.CLUSTER_ERR_CAP, _lib.CLUSTER_ERR_ROWS)
    assert sum(bits) == (1 << len(bits)) - 1                          # eight disjoint bits of one word


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_cluster_kernels_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "voxel_cluster.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
