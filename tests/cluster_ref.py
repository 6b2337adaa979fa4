"""numpy restatement of the Euclidean-clustering rule (include/pn2.h, ``pn2_voxel_components``), for the tests.

The voxels of ONE cloud (what ``voxel_ref.voxel_grid`` returns) are grouped by cell through a dict; two voxels that take part
are adjacent iff their cells differ by a vector of {-1, 0, 1}^3 \\ {0} with at most 1 / 2 / 3 non-zero entries (connectivity 6 /
18 / 26), no cell outside ``[-2**20, 2**20)`` exists, and with ``same_label`` their labels are equal; a host union-find makes the
components; the kept ones (``points >= min_points`` and ``voxels >= min_voxels``) are numbered in ascending order of their root,
the lowest voxel rank.  Shares no code with the kernel.
"""
import itertools

import numpy as np

import voxel_ref as VR

LIMIT = 1 << 20
NONZERO = {6: 1, 18: 2, 26: 3}


def offsets(connectivity):
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(x != 0 for x in d) <= NONZERO[connectivity]]


def takes_part(vox_labels, member, V):
    if vox_labels is None:
        return np.ones(V, bool)
    lab = np.asarray(vox_labels).astype(np.int64)
    part = lab >= 0
    if member is not None:
        member = np.asarray(member)
        inside = part & (lab < len(member))
        part = inside.copy()
        part[inside] = member[lab[inside]] != 0
    return part


def components_of_cells(cells, n_points, vox_labels=None, connectivity=26, same_label=True, member=None, min_points=1, min_voxels=1,
                        valid=None):
    """The rule on one cloud's voxels: ``cells`` int ``[V, 3]`` in rank order (distinct), ``n_points`` ``[V]``.  ``valid``: bool
    ``[V]``, False where the representative's cell is invalid (the voxel takes no part).  Returns a dict: ``vox_component`` int32
    ``[V]``, ``count``, ``root`` / ``points`` / ``voxels`` / ``label`` int32 per kept component, and ``part_root`` int64 ``[V]``: the root of
    every voxel's component, kept or not (-1: takes no part)."""
    cells = np.asarray(cells).astype(np.int64).reshape(-1, 3)
    V = len(cells)
    part = takes_part(vox_labels, member, V)
    if valid is not None:
        part &= np.asarray(valid, bool)
    where = {tuple(c): v for v, c in enumerate(cells.tolist()) if part[v]}
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    offs = offsets(connectivity)
    for cell, v in where.items():
        for d in offs:
            n = (cell[0] + d[0], cell[1] + d[1], cell[2] + d[2])
            if not all(-LIMIT <= x < LIMIT for x in n):
                continue
            u = where.get(n)
            if u is None or (same_label and vox_labels is not None and vox_labels[u] != vox_labels[v]):
                continue
            a, b = find(v), find(u)
            if a != b:
                parent[max(a, b)] = min(a, b)
    part_root = np.array([find(v) if part[v] else -1 for v in range(V)], np.int64)
    n_points = np.asarray(n_points).astype(np.int64)
    roots = np.unique(part_root[part_root >= 0])                    # ascending: the numbering rule
    lowest = np.full(V + 1, V, np.int64)
    np.minimum.at(lowest, part_root[part_root >= 0], np.flatnonzero(part_root >= 0))
    assert np.array_equal(lowest[roots], roots)                      # a root IS the lowest rank of its component
    points = np.bincount(part_root[part_root >= 0], weights=n_points[part_root >= 0], minlength=max(V, 1))[roots].astype(np.int64)
    voxels = np.bincount(part_root[part_root >= 0], minlength=max(V, 1))[roots]
    kept = (points >= min_points) & (voxels >= min_voxels)
    ident = np.full(V + 1, -1, np.int64)
    ident[roots[kept]] = np.arange(int(kept.sum()))
    vox_component = np.where(part_root >= 0, ident[part_root], -1).astype(np.int32)
    lab = np.zeros(V, np.int32) if vox_labels is None else np.asarray(vox_labels).astype(np.int32)
    return {"vox_component": vox_component, "count": int(kept.sum()), "root": roots[kept].astype(np.int32),
            "points": points[kept].astype(np.int32), "voxels": voxels[kept].astype(np.int32), "label": lab[roots[kept]],
            "part_root": part_root}


def rows_of(vox_component, inverse, vox_labels=None, row_labels=None):
    """``row_component``: -1 where ``inverse < 0``; else the voxel's id; with ``row_labels``, -1 where the row's label differs from its
    voxel's."""
    inverse = np.asarray(inverse).astype(np.int64)
    out = np.full(len(inverse), -1, np.int32)
    has = inverse >= 0
    out[has] = np.asarray(vox_component)[inverse[has]]
    if row_labels is not None:
        differs = has.copy()
        differs[has] = np.asarray(row_labels)[has] != np.asarray(vox_labels)[inverse[has]]
        out[differs] = -1
    return out


def cluster(points, origin, voxel, vox_labels=None, row_labels=None, grid=None, **rule):
    """One cloud ``[M, ld]``: ``voxel_ref.voxel_grid`` (or a given ``grid`` dict of it), then the rule.  The cells are those of the
    representative rows.  Adds ``row_component`` and ``grid`` to ``components_of_cells``'s dict."""
    grid = VR.voxel_grid(points, origin, voxel) if grid is None else grid
    q, valid = VR.cells(np.asarray(points, np.float32)[grid["index"]], origin, voxel)
    cells = np.where(valid[:, None], q, 0.0).astype(np.int64)
    out = components_of_cells(cells, grid["n_points"], vox_labels, valid=valid, **rule)
    out["row_component"] = rows_of(out["vox_component"], grid["inverse"], vox_labels, row_labels)
    out["grid"] = grid
    return out


def snake_cells(n, width=25):
    """A one-cell-wide serpentine path of ``n`` cells in the plane z = 0: rows of ``width`` cells along x at every second y,
    joined by single cells alternately at the right and the left end.  Consecutive cells share a face; no other pair of cells does."""
    cells = []
    x, y, step = 0, 0, 1
    while len(cells) < n:
        for _ in range(width):
            cells.append((x, y, 0))
            x += step
        x -= step
        cells.append((x, y + 1, 0))
        y += 2
        step = -step
    return np.array(cells[:n], np.int64)
