"""GPU: Euclidean clustering on the voxel grid (``pn2_voxel_components``, csrc/voxel_cluster.hip; ``voxel.VoxelGrid.components``,
``voxel.euclidean_cluster``, ``FrameSegmenter.label_scan(instances=)``) against the numpy statement of its rule
(tests/cluster_ref.py), EXACTLY.  Every ABI call runs with poisoned outputs and a 0xEE-filled workspace (``run_abi``): every entry
outside the clouds' rows, voxels and components must come back untouched.  The grid a call starts from (``out_index``, ``n_points``,
``inverse``, the counts) is the numpy statement's (tests/voxel_ref.py), so nothing here depends on ``pn2_voxel_grid``."""
import ctypes

import numpy as np
import pytest
import torch

import cluster_ref as R
import scan_filter_ref as SR
import voxel_reduce_ref as RR
import voxel_ref as VR
from conftest import golden
from pointnet12_amd import _lib, kitti, voxel
from pointnet12_amd import kitti_view as V

pytestmark = pytest.mark.gpu

T = _lib.VOXEL_TILE
POISON = -777
PER_COMPONENT = ("root", "points", "voxels", "label")
# site occupancies just above the percolation thresholds of the simple cubic lattice with 6 / 18 / 26 neighbours (0.312, 0.137,
# 0.098): chosen on the CPU with the restatement so that at 5000 voxels one component spans every tile of the compaction while
# hundreds of voxels stay alone (6: 908 components, the largest of 1678 voxels, 548 singletons; 18: 445 / 3601 / 256; 26: 491 /
# 3037 / 274)
DENSITY = {6: 0.36, 18: 0.17, 26: 0.12}
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 5000]


def rows_of_cells(cells, rng=None, extra=0, ld=4):
    """Float32 rows at ``voxel = 1``: row v lies in the middle of cell v (exact in float32 up to the grid's ends), then ``extra`` more
    rows in randomly chosen cells.  The voxel of rank v is cell v."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    pick = np.arange(len(cells))
    if extra:
        pick = np.concatenate([pick, rng.integers(0, len(cells), extra)])
    pts = np.zeros((len(pick), ld), np.float32)
    pts[:, :3] = cells[pick] + 0.5
    assert np.array_equal(np.floor(pts[:, :3].astype(np.float64)), cells[pick])
    return pts


def random_cells(rng, Vn, density):
    side = int(np.ceil((Vn / density) ** (1.0 / 3.0)))
    flat = rng.choice(side ** 3, Vn, replace=False)
    return np.stack([flat % side, (flat // side) % side, flat // (side * side)], 1) - side // 2


def grid_of(pts, vox=1.0, origin=0.0):
    if len(pts) == 0:
        e = np.zeros(0, np.int32)
        return {"index": e, "n_points": e, "inverse": e, "count": 0}
    return VR.voxel_grid(pts, origin, vox)


def run_abi(dev, clouds, vox=1.0, origin=0.0, max_rows=None, connectivity=26, same_label=True, member=None, min_points=1, min_voxels=1,
            want=("vox", "row") + PER_COMPONENT, expect_rc=0):
    """One ``pn2_voxel_components`` call.  ``clouds``: dicts with ``pts`` ``[M, ld]`` and optionally ``vox_labels`` ``[V]``, ``row_labels``
    ``[M]``, ``grid`` (else ``voxel_ref.voxel_grid``), ``rows`` / ``voxels`` (device-side counts other than M / V).  The rows, voxels
    and components of the clouds lie back to back with DIFFERENT gaps.  Returns ``(per-cloud dicts, err)``."""
    lib = _lib.load()
    B, ld = len(clouds), clouds[0]["pts"].shape[1]
    grids = [c.get("grid") or grid_of(c["pts"], vox, origin) for c in clouds]
    Ms, Vs = [len(c["pts"]) for c in clouds], [g["count"] for g in grids]
    max_rows = max(Ms) if max_rows is None else max_rows
    row_begin, out_begin, comp_begin = [], [], []
    r, o, k = 3, 5, 11
    for M, Vn in zip(Ms, Vs):
        row_begin.append(r), out_begin.append(o), comp_begin.append(k)
        r, o, k = r + M + 2, o + Vn + 7, k + Vn + 1
    rows, vrows, crows = r + 4, o + 4, k + 4
    pts = np.full((rows, ld), 1e30, np.float32)
    inverse, row_labels = np.full(rows, 1 << 30, np.int32), np.full(rows, 5, np.int32)
    index, n_points, vox_labels = np.full(vrows, 1 << 30, np.int32), np.full(vrows, 1 << 20, np.int32), np.full(vrows, 0, np.int32)
    labelled, by_row = "vox_labels" in clouds[0], "row_labels" in clouds[0]
    for b, (c, g) in enumerate(zip(clouds, grids)):
        pts[row_begin[b]:row_begin[b] + Ms[b]] = c["pts"]
        inverse[row_begin[b]:row_begin[b] + Ms[b]] = g["inverse"]
        index[out_begin[b]:out_begin[b] + Vs[b]] = g["index"]
        n_points[out_begin[b]:out_begin[b] + Vs[b]] = g["n_points"]
        if labelled:
            vox_labels[out_begin[b]:out_begin[b] + Vs[b]] = c["vox_labels"]
        if by_row:
            row_labels[row_begin[b]:row_begin[b] + Ms[b]] = c["row_labels"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)
    d = {"pts": up(pts), "inverse": up(inverse), "index": up(index), "n_points": up(n_points), "row_begin": t64(row_begin),
         "row_count": t64([c.get("rows", M) for c, M in zip(clouds, Ms)]), "out_begin": t64(out_begin),
         "out_count": t64([c.get("voxels", Vn) for c, Vn in zip(clouds, Vs)]), "comp_begin": t64(comp_begin),
         "vox_labels": up(vox_labels) if labelled else None, "row_labels": up(row_labels) if by_row else None,
         "member": None if member is None else up(np.asarray(member, np.int32))}
    for c, M, Vn in zip(clouds, Ms, Vs):                              # (the arrays made above hold no more than M rows, V voxels)
        assert min(c.get("rows", M), max_rows) <= M and min(c.get("voxels", Vn), max_rows) <= Vn
    poison = lambda n: torch.full((n,), POISON, dtype=torch.int32, device=dev)
    o_vox, o_row = poison(vrows), poison(rows)
    o_comp = {name: poison(crows) for name in PER_COMPONENT}
    cnt = torch.full((B,), -5, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = lib.pn2_voxel_components_workspace_bytes(B, max_rows)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    org_a, vox_a = np.ascontiguousarray(VR.triple(origin)), np.ascontiguousarray(VR.triple(vox))
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p = _lib.ptr
    opt = lambda name, t: p(t) if name in want else None
    rc = lib.pn2_voxel_components(p(d["pts"]), ld, p(d["row_begin"]), p(d["row_count"]), B, max_rows, dp(org_a), dp(vox_a), p(d["out_begin"]),
                                  p(d["out_count"]), p(d["index"]), p(d["n_points"]), p(d["vox_labels"]), p(d["inverse"]), p(d["row_labels"]),
                                  connectivity, 1 if same_label else 0, p(d["member"]), 0 if member is None else len(member), min_points,
                                  min_voxels, p(d["comp_begin"]), opt("vox", o_vox), opt("row", o_row), opt("root", o_comp["root"]),
                                  opt("points", o_comp["points"]), opt("voxels", o_comp["voxels"]), opt("label", o_comp["label"]), p(cnt),
                                  p(err), p(ws), _lib.stream())
    assert rc == expect_rc
    torch.cuda.synchronize()
    vox_h, row_h, cnt_h = o_vox.cpu().numpy(), o_row.cpu().numpy(), cnt.cpu().numpy()
    comp_h = {name: t.cpu().numpy() for name, t in o_comp.items()}
    if rc != 0:                                                      # refused: nothing was launched, nothing written
        assert (vox_h == POISON).all() and (row_h == POISON).all() and (cnt_h == -5).all()
        assert all((a == POISON).all() for a in comp_h.values()) and (ws.cpu().numpy() == 0xEE).all()
        return None, 0
    seen_v, seen_r, seen_c = np.zeros(vrows, bool), np.zeros(rows, bool), np.zeros(crows, bool)
    got = []
    for b in range(B):
        nr = max(0, min(clouds[b].get("rows", Ms[b]), max_rows))
        nv = max(0, min(clouds[b].get("voxels", Vs[b]), max_rows))
        n = int(cnt_h[b])
        assert 0 <= n <= nv
        seen_r[row_begin[b]:row_begin[b] + nr] = True
        seen_v[out_begin[b]:out_begin[b] + nv] = True
        seen_c[comp_begin[b]:comp_begin[b] + n] = True
        one = {"count": n, "vox_component": vox_h[out_begin[b]:out_begin[b] + nv], "row_component": row_h[row_begin[b]:row_begin[b] + nr]}
        one.update({name: comp_h[name][comp_begin[b]:comp_begin[b] + n] for name in PER_COMPONENT})
        got.append(one)
    assert (vox_h[~seen_v] == POISON).all() if "vox" in want else (vox_h == POISON).all(), "vox_component written outside the voxels"
    assert (row_h[~seen_r] == POISON).all() if "row" in want else (row_h == POISON).all(), "row_component written outside the rows"
    for name in PER_COMPONENT:
        assert (comp_h[name][~seen_c] == POISON).all() if name in want else (comp_h[name] == POISON).all(), name
    return got, int(err.item())


def compare(ref, got, want=("vox", "row") + PER_COMPONENT):
    assert got["count"] == ref["count"]
    if "vox" in want:
        assert np.array_equal(got["vox_component"], ref["vox_component"])
    if "row" in want:
        assert np.array_equal(got["row_component"], ref["row_component"])
    for name in PER_COMPONENT:
        if name in want:
            assert np.array_equal(got[name], ref[name]), name


def reference(cloud, vox=1.0, origin=0.0, **rule):
    return R.cluster(cloud["pts"], origin, vox, cloud.get("vox_labels"), cloud.get("row_labels"), grid=cloud.get("grid"), **rule)


def run_and_compare(dev, cloud, **kw):
    """One cloud through ``run_abi`` and ``compare``, the cap bit and every other bit clear; returns the reference."""
    rule = {k: kw[k] for k in ("connectivity", "same_label", "member", "min_points", "min_voxels") if k in kw}
    ref = reference(cloud, kw.get("vox", 1.0), kw.get("origin", 0.0), **rule)
    got, err = run_abi(dev, [cloud], **kw)
    assert err == 0
    compare(ref, got[0], kw.get("want", ("vox", "row") + PER_COMPONENT))
    return ref


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("Vn", SIZES)
def test_sizes_near_the_percolation_threshold(dev, Vn, connectivity):
    rng = np.random.default_rng(Vn)
    cells = random_cells(rng, Vn, DENSITY[connectivity])
    cloud = {"pts": rows_of_cells(cells, rng, extra=Vn // 2 + 3)}
    ref = run_and_compare(dev, cloud, connectivity=connectivity)
    assert ref["grid"]["count"] == Vn and ref["points"].sum() == len(cloud["pts"])
    if Vn == 5000:
        largest = np.flatnonzero(ref["vox_component"] == ref["voxels"].argmax())
        assert len(set((largest // T).tolist())) == 5 and len(largest) > 1500 and (ref["voxels"] == 1).sum() > 200


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_snake(dev, order):
    """A one-cell-wide path of 20 000 voxels: ONE component however the rows are ordered -- in ascending order every voxel links to
    its predecessor, the deepest forest there is -- and the cap bit stays clear; cut once, two components numbered by their roots."""
    n = 20000
    cells = R.snake_cells(n)
    perm = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.default_rng(1).permutation(n)}[order]
    ref = run_and_compare(dev, {"pts": rows_of_cells(cells[perm])}, connectivity=6)
    assert ref["count"] == 1 and ref["voxels"].tolist() == [n] and ref["root"].tolist() == [0] and not ref["row_component"].any()
    cut = np.delete(cells, 12345, 0)[perm[perm < n - 1]]
    ref = run_and_compare(dev, {"pts": rows_of_cells(cut)}, connectivity=6)
    assert ref["count"] == 2 and sorted(ref["voxels"].tolist()) == [n - 1 - 12345, 12345]
    ref = run_and_compare(dev, {"pts": rows_of_cells(cut)}, connectivity=6, min_voxels=12345)
    assert ref["count"] == 1 and ref["voxels"].tolist() == [12345] and (ref["vox_component"] == -1).sum() == n - 1 - 12345


def test_extremes(dev):
    rng = np.random.default_rng(2)
    M = 3 * T + 5
    one = np.zeros((M, 4), np.float32)
    one[:, :3] = rng.uniform(0.01, 0.99, size=(M, 3)).astype(np.float32)             # every row in ONE voxel
    ref = run_and_compare(dev, {"pts": one})
    assert ref["count"] == 1 and ref["points"].tolist() == [M] and ref["voxels"].tolist() == [1]
    run_and_compare(dev, {"pts": one}, min_points=M + 1)                             # ... and not kept
    i = rng.permutation(M)                                                           # every voxel isolated: max_rows = M voxels, the
    cells = np.stack([i % 17, (i // 17) % 17, i // 289], 1) * 2 - 9                  # table at its highest load
    for c in (6, 26):
        ref = run_and_compare(dev, {"pts": rows_of_cells(cells)}, connectivity=c, max_rows=M)
        assert ref["count"] == M and np.array_equal(ref["root"], np.arange(M)) and np.array_equal(ref["row_component"], np.arange(M))
    full = np.stack(np.meshgrid(np.arange(13), np.arange(12), np.arange(11), indexing="ij"), -1).reshape(-1, 3)       # a full block
    ref = run_and_compare(dev, {"pts": rows_of_cells(full[rng.permutation(len(full))])}, connectivity=6)
    assert ref["count"] == 1 and ref["voxels"].tolist() == [13 * 12 * 11]


def test_axis_ends_are_no_neighbours(dev):
    top, low = (1 << 20) - 1, -(1 << 20)
    for a, b in ((2, 1), (1, 0)):                                    # the z / y boundary of the packed key, then the y / x one
        def cell(hi, lo_axis_value, base=7):
            c = [base, base, base]
            c[b], c[a] = hi, lo_axis_value
            return tuple(c)
        # keys that differ by 1: (.., k, top) and (.., k + 1, low); true neighbours: (.., top - 1) and (.., top); and the same at the
        # low end, with a cell across the far end of the axis
        cells = [cell(0, top), cell(1, low), cell(3, top - 1), cell(3, top), cell(5, low), cell(5, low + 1), cell(5, top)]
        for c in (6, 18, 26):
            ref = run_and_compare(dev, {"pts": rows_of_cells(cells)}, connectivity=c)
            assert ref["vox_component"].tolist() == [0, 1, 2, 2, 3, 3, 4]
    corners = [(top, top, top), (low, low, low), (top, low, top), (top - 1, top - 1, top - 1), (low + 1, low, low + 1)]
    assert [run_and_compare(dev, {"pts": rows_of_cells(corners)}, connectivity=c)["count"] for c in (6, 18, 26)] == [5, 4, 3]


def test_diagonals_split_the_connectivities(dev):
    cells = [(0, 0, 0), (1, 1, 0), (2, 2, 1), (5, 5, 5), (5, 5, 6), (-3, 0, 0), (-4, -1, 0), (-4, -2, -1), (-4, -2, -3)]
    counts = []
    for c in (6, 18, 26):
        ref = run_and_compare(dev, {"pts": rows_of_cells(cells)}, connectivity=c)
        counts.append(ref["count"])
    assert counts == [8, 5, 4]
    # every one of the 26 offsets on its own, from both sides: a pair is joined iff the connectivity reaches that far
    for d in R.offsets(26):
        pair = [(10, 10, 10), (10 + d[0], 10 + d[1], 10 + d[2])]
        for c in (6, 18, 26):
            want = 1 if sum(x != 0 for x in d) <= R.NONZERO[c] else 2
            assert run_and_compare(dev, {"pts": rows_of_cells(pair)}, connectivity=c)["count"] == want
            assert run_and_compare(dev, {"pts": rows_of_cells(pair[::-1])}, connectivity=c)["count"] == want


def test_labels_member_and_the_row_rule(dev):
    rng = np.random.default_rng(4)
    Vn = 2 * T + 9
    cells = random_cells(rng, Vn, 0.5)                              # half full: one component without labels
    pts = rows_of_cells(cells, rng, extra=Vn)
    grid = grid_of(pts)
    left = cells[:, 0] < 0
    vox_labels = np.where(left, 2, 3).astype(np.int32)              # a label border at x = 0
    base = {"pts": pts, "grid": grid}
    assert run_and_compare(dev, base)["count"] == 1
    on = run_and_compare(dev, dict(base, vox_labels=vox_labels), same_label=True)
    off = run_and_compare(dev, dict(base, vox_labels=vox_labels), same_label=False)
    assert on["count"] >= 2 and off["count"] == 1 and set(on["label"].tolist()) == {2, 3}
    # member with zeros, labels of -1 and at or beyond L = 4
    mixed = vox_labels.copy()
    mixed[rng.random(Vn) < 0.1] = -1
    mixed[rng.random(Vn) < 0.1] = 4
    mixed[rng.random(Vn) < 0.1] = 1 << 30
    mixed[rng.random(Vn) < 0.1] = 0
    for member in (None, [0, 1, 1, 0], [1, 0, 0, 1], [0, 0, 0, 0]):
        for same in (True, False):
            ref = run_and_compare(dev, dict(base, vox_labels=mixed), member=member, same_label=same)
            part = (mixed >= 0) if member is None else np.isin(mixed, np.flatnonzero(member))
            assert np.array_equal(ref["vox_component"] >= 0, part)
    # rows that disagree with their voxel get -1, voxels and components stay what they were
    row_labels = mixed[grid["inverse"]].copy()
    flip = rng.random(len(pts)) < 0.2
    row_labels[flip] = 7
    ref = run_and_compare(dev, dict(base, vox_labels=mixed, row_labels=row_labels), member=[0, 0, 1, 1])
    plain = reference(dict(base, vox_labels=mixed), member=[0, 0, 1, 1])
    assert np.array_equal(ref["vox_component"], plain["vox_component"]) and (ref["row_component"][flip] == -1).all()
    assert np.array_equal(ref["row_component"][~flip], plain["row_component"][~flip]) and (plain["row_component"][flip] >= 0).any()


def test_thresholds_exactly_at_the_size(dev):
    # three bars: 5 voxels / 9 rows, 3 voxels / 3 rows, 4 voxels / 12 rows; one lone voxel of 6 rows
    cells = [(x, 0, 0) for x in range(5)] + [(x, 5, 0) for x in range(3)] + [(x, 9, 0) for x in range(4)] + [(0, 20, 0)]
    extra = [0] * 4 + [8, 9, 10, 11] * 2 + [12] * 5
    pts = np.concatenate([rows_of_cells(cells), rows_of_cells(cells)[extra]], 0)
    sizes = {"points": [9, 3, 12, 6], "voxels": [5, 3, 4, 1]}
    ref = run_and_compare(dev, {"pts": pts})
    assert ref["points"].tolist() == sizes["points"] and ref["voxels"].tolist() == sizes["voxels"]
    for name, arg in (("points", "min_points"), ("voxels", "min_voxels")):
        for k, size in enumerate(sizes[name]):
            for delta in (-1, 0, 1):
                if size + delta < 1:
                    continue
                ref = run_and_compare(dev, {"pts": pts}, **{arg: size + delta})
                keep = [s >= size + delta for s in sizes[name]]
                assert keep[k] == (delta <= 0) and ref["count"] == sum(keep)
                assert ref["root"].tolist() == [r for r, kept in zip((0, 5, 8, 12), keep) if kept]           # ids stay in root order
    ref = run_and_compare(dev, {"pts": pts}, min_points=6, min_voxels=4)
    assert ref["root"].tolist() == [0, 8] and ref["vox_component"].tolist() == [0] * 5 + [-1] * 3 + [1] * 4 + [-1]


def test_batches(dev):
    rng = np.random.default_rng(6)
    cells = random_cells(rng, T + 40, DENSITY[26])
    a = {"pts": rows_of_cells(cells, rng, extra=100)}
    clouds = [a, {"pts": np.zeros((0, 4), np.float32)}, {"pts": a["pts"].copy()}, {"pts": rows_of_cells(cells[:200][::-1])}]
    refs = [reference(c) if len(c["pts"]) else None for c in clouds]
    # max_rows above every count; comp_begin differs from out_begin (run_abi's layout); an empty cloud; equal coordinates twice
    got, err = run_abi(dev, clouds, max_rows=2 * T + 100)
    assert err == 0 and got[1]["count"] == 0 and got[0]["count"] == got[2]["count"] > 10
    for b in (0, 2, 3):
        compare(refs[b], got[b])
    # labelled, with member, in a batch
    labelled = [dict(c, vox_labels=rng.integers(-1, 3, grid_of(c["pts"])["count"]).astype(np.int32)) for c in clouds]
    got, err = run_abi(dev, labelled, max_rows=T + 140, member=[1, 0, 1], connectivity=18)
    assert err == 0
    for b in (0, 2, 3):
        compare(reference(labelled[b], member=[1, 0, 1], connectivity=18), got[b])
    # each optional output NULL in turn, and the count alone
    every = ("vox", "row") + PER_COMPONENT
    for missing in every:
        want = tuple(n for n in every if n != missing)
        got, err = run_abi(dev, clouds, want=want)
        for b in (0, 2, 3):
            compare(refs[b], got[b], want)
    got, err = run_abi(dev, clouds, want=())
    assert err == 0 and [g["count"] for g in got] == [refs[0]["count"], 0, refs[2]["count"], refs[3]["count"]]


def test_error_bits(dev):
    rng = np.random.default_rng(8)
    cells = random_cells(rng, 300, 0.3)
    pts = rows_of_cells(cells, rng, extra=50)
    grid = grid_of(pts)
    # an out_index outside the cloud's rows: that voxel takes no part, the rest is the rule's
    bad = dict(grid, index=grid["index"].copy())
    bad["index"][[7, 120]] = (len(pts), -1)
    got, err = run_abi(dev, [{"pts": pts, "grid": bad}])
    valid = np.ones(300, bool)
    valid[[7, 120]] = False
    ref = R.components_of_cells(cells, grid["n_points"], valid=valid)
    assert err == _lib.CLUSTER_ERR_INDEX and np.array_equal(got[0]["vox_component"], ref["vox_component"])
    assert (got[0]["vox_component"][[7, 120]] == -1).all()
    # an inverse at or beyond the voxel count: the row gets -1
    bad = dict(grid, inverse=grid["inverse"].copy())
    bad["inverse"][[3, 33]] = (300, 1 << 30)
    got, err = run_abi(dev, [{"pts": pts, "grid": bad}])
    want = R.cluster(pts, 0.0, 1.0)["row_component"].copy()
    want[[3, 33]] = -1
    assert err == _lib.CLUSTER_ERR_INDEX and np.array_equal(got[0]["row_component"], want)
    # a representative row outside the grid
    off = pts.copy()
    off[grid["index"][5], 0] = np.nan
    got, err = run_abi(dev, [{"pts": off, "grid": grid}])
    valid = np.ones(300, bool)
    valid[5] = False
    assert err == _lib.CLUSTER_ERR_CELL
    assert np.array_equal(got[0]["vox_component"], R.components_of_cells(cells, grid["n_points"], valid=valid)["vox_component"])
    # counts above max_rows: clamped, the bit set, nothing beyond is touched (run_abi checks that)
    bare = rows_of_cells(cells)                                     # (as many rows as voxels: max_rows clamps both counts to the truth)
    for over in ({"rows": 10 ** 9}, {"voxels": 301}, {"rows": 1 << 40, "voxels": 1 << 40}):
        got, err = run_abi(dev, [dict({"pts": bare}, **over)], max_rows=300)
        assert err == _lib.CLUSTER_ERR_ROWS
        compare(R.cluster(bare, 0.0, 1.0), got[0])
    got, err = run_abi(dev, [{"pts": pts, "grid": grid, "rows": -4, "voxels": -4}])
    assert err == 0 and got[0]["count"] == 0


def test_invalid_arguments_launch_nothing(dev):
    cloud = {"pts": rows_of_cells(random_cells(np.random.default_rng(0), 100, 0.3))}
    cloud["grid"] = grid_of(cloud["pts"])
    EINVAL = -1
    for kw in ({"connectivity": 0}, {"connectivity": 8}, {"connectivity": 27}, {"connectivity": -26}, {"min_points": 0}, {"min_voxels": 0},
               {"min_voxels": -1}, {"member": [1, 1]}, {"vox": 0.0}, {"vox": float("nan")}, {"origin": float("inf")}, {"max_rows": -1},
               {"max_rows": _lib.VOXEL_MAX_ROWS + 1}):
        if "max_rows" in kw:
            assert _lib.load().pn2_voxel_components_workspace_bytes(1, kw["max_rows"]) == EINVAL
            continue
        run_abi(dev, [cloud], expect_rc=EINVAL, **kw)                # (member without the voxels' labels is one of them)
    run_abi(dev, [dict(cloud, row_labels=np.zeros(100, np.int32))], expect_rc=EINVAL)           # row_labels without them too
    run_abi(dev, [dict(cloud, pts=cloud["pts"][:, :2])], expect_rc=EINVAL)                      # ld = 2


def test_same_bytes_twice_and_on_reversed_input(dev):
    rng = np.random.default_rng(9)
    Vn = 30000
    cells = random_cells(rng, Vn, DENSITY[26])
    pts = rows_of_cells(cells, rng, extra=Vn)
    runs = [run_abi(dev, [{"pts": pts}])[0][0] for _ in range(2)]
    for name in ("vox_component", "row_component") + PER_COMPONENT:
        assert runs[0][name].tobytes() == runs[1][name].tobytes(), name
    ref = R.cluster(pts, 0.0, 1.0)
    compare(ref, runs[0])
    back_ref = run_and_compare(dev, {"pts": pts[::-1]})              # the numbering rule's ids on the reversed input
    assert back_ref["count"] == ref["count"] > 100
    # the same partition: rows i and M - 1 - i name each other's components one to one, with equal sizes
    pairs = set(zip(ref["row_component"].tolist(), back_ref["row_component"][::-1].tolist()))
    assert len(pairs) == ref["count"]
    assert sorted(ref["points"].tolist()) == sorted(back_ref["points"].tolist())


# ------------------------------------------------------------------------------------------------------------- the Python layer

def one_cloud(rng, Vn, density, vox, labels=True):
    cells = random_cells(rng, Vn, density)
    pts = rows_of_cells(cells, rng, extra=2 * Vn)
    pts[:, :3] *= np.float32(vox)                                   # (vox a power of two: still exact)
    pts[:, 3] = rng.normal(size=len(pts)).astype(np.float32)
    row_labels = None
    if labels:
        row_labels = np.where(pts[:, 0] < 0, 1, 4).astype(np.int32)
        row_labels[rng.random(len(pts)) < 0.15] = 6
        row_labels[rng.random(len(pts)) < 0.05] = -1
    return pts, row_labels


def mode_grid(pts, row_labels, vox):
    """The numpy statement of ``VoxelGrid(label_reduce="mode").downsample``'s labels."""
    grid = VR.voxel_grid(pts, 0.0, vox)
    winner, _, _ = RR.segment_mode(row_labels, grid["inverse"], grid["count"], -1)
    return grid, winner.astype(np.int32)


def tuple_to_dict(comps, rows, voxels, b0=0, v0=0, c0=0, b=0):
    n = int(comps.count[b].item())
    cpu = lambda t, lo, m: t[lo:lo + m].cpu().numpy()
    return {"count": n, "row_component": cpu(comps.row_component, b0, rows), "vox_component": cpu(comps.voxel_component, v0, voxels),
            "root": cpu(comps.root, c0, n), "points": cpu(comps.n_points, c0, n), "voxels": cpu(comps.n_voxels, c0, n),
            "label": cpu(comps.label, c0, n)}


def test_components_and_euclidean_cluster(dev):
    rng = np.random.default_rng(12)
    pts, row_labels = one_cloud(rng, 3000, 0.3, 0.25)
    grid, vox_labels = mode_grid(pts, row_labels, 0.25)
    member = [0, 1, 0, 0, 1]
    ref = R.cluster(pts, 0.0, 0.25, vox_labels, row_labels, grid=grid, member=member, min_points=4, connectivity=18)
    assert ref["count"] > 10 and (ref["row_component"] == -1).any()
    pts_d, lab_d = torch.from_numpy(pts).to(dev), torch.from_numpy(row_labels).to(dev)
    vg = voxel.VoxelGrid(0.25, device=dev, label_reduce="mode")
    down = vg.downsample(pts_d, lab_d)
    comps = vg.components(pts_d, down, row_labels=lab_d, connectivity=18, member=member, min_points=4)
    vg.check()
    assert isinstance(comps, voxel.Components) and comps.count.dtype == torch.int64 and comps.count.is_cuda
    compare(ref, tuple_to_dict(comps, len(pts), grid["count"]))
    both, down2, grid2 = voxel.euclidean_cluster(pts_d, lab_d, voxel_size=0.25, connectivity=18, member=member, min_points=4)
    grid2.check()
    compare(ref, tuple_to_dict(both, len(pts), grid["count"]))
    # without labels every voxel takes part; the [B, M, ld] form
    cube = np.ascontiguousarray(np.stack([pts[:2000], pts[1000:3000], pts[:2000][::-1]], 0))
    comps, down, g3 = voxel.euclidean_cluster(torch.from_numpy(cube).to(dev), voxel_size=0.25, connectivity=6)
    g3.check()
    for b in range(3):
        r = R.cluster(cube[b], 0.0, 0.25, connectivity=6)
        compare(r, tuple_to_dict(comps, 2000, r["grid"]["count"], b * 2000, b * 2000, b * 2000, b))
    with pytest.raises(ValueError):
        vg.components(pts_d, down, connectivity=12)
    with pytest.raises(ValueError):
        voxel.euclidean_cluster(pts_d, None, voxel_size=0.25, member=member)


def test_centroids_through_segment_mean(dev):
    rng = np.random.default_rng(13)
    pts, _ = one_cloud(rng, 2000, DENSITY[26], 0.5, labels=False)
    ref = R.cluster(pts, 0.0, 0.5, min_points=3)
    pts_d = torch.from_numpy(pts).to(dev)
    comps, down, grid = voxel.euclidean_cluster(pts_d, voxel_size=0.5, min_points=3)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    mean = voxel.segment_mean(pts_d, comps.row_component, comps.count, error_flag=err)
    n = ref["count"]
    assert int(comps.count.item()) == n > 20 and int(err.item()) == 0
    want = RR.segment_mean(pts, ref["row_component"], n)             # the existing rule's bits
    assert np.array_equal(mean[:n].cpu().numpy().view(np.uint32), want["mean"].view(np.uint32))
    plain = np.stack([pts[ref["row_component"] == i].astype(np.float64).mean(0) for i in range(n)], 0)
    # numpy's fp64 centroids: the rule truncates every term by at most 2^-33 of the column's largest magnitude and rounds once to float32
    assert np.abs(mean[:n].cpu().numpy() - plain).max() <= 2.0 ** -23 * np.abs(pts).max()
    labels = torch.from_numpy((pts[:, 0] > 0).astype(np.int32)).to(dev)
    mode = voxel.segment_mode(labels, comps.row_component, comps.count)
    winner, _, _ = RR.segment_mode(labels.cpu().numpy(), ref["row_component"], n, -1)
    assert np.array_equal(mode[:n].cpu().numpy(), winner)


def test_capture_and_replay_with_other_counts(dev):
    rng = np.random.default_rng(14)
    cap = 4 * T + 17
    clouds = []
    for Vn in (T, 700, T + 300):
        p, l = one_cloud(rng, Vn, 0.3, 0.5)
        assert len(p) <= cap
        clouds.append((p, l))
    vg = voxel.VoxelGrid(0.5, device=dev, label_reduce="mode")
    bufs, cbufs = vg.buffers(cap), vg.component_buffers(cap)
    pts_s = torch.zeros(cap, 4, device=dev)
    lab_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    begin = torch.zeros(1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    member = torch.tensor([0, 1, 0, 0, 1], dtype=torch.int32, device=dev)

    def load(p, l):
        pts_s[:len(p)].copy_(torch.from_numpy(p))
        lab_s[:len(p)].copy_(torch.from_numpy(l))
        count.fill_(len(p))

    def step():
        down = vg.downsample(pts_s, lab_s, begin, count, cap, out=bufs)
        return vg.components(pts_s, down, row_labels=lab_s, member=member, min_voxels=2, row_begin=begin, row_count=count, max_rows=cap,
                             out=cbufs)

    load(*clouds[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        comps = step()
    for p, l in (clouds[1], clouds[2], clouds[0], (clouds[1][0][:T - 1], clouds[1][1][:T - 1])):
        load(p, l)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before               # nothing allocated by a replay
        grid, vox_labels = mode_grid(p, l, 0.5)
        ref = R.cluster(p, 0.0, 0.5, vox_labels, l, grid=grid, member=[0, 1, 0, 0, 1], min_voxels=2)
        assert ref["count"] > 3
        compare(ref, tuple_to_dict(comps, len(p), grid["count"]))
        assert int(vg.error_flag.item()) == 0


class Stub(torch.nn.Module):
    """A tiny stand-in for the network: ``[1, 4, n]`` -> log-probabilities ``[1, n, 19]``, constant over blocks of 4 m in x and y so
    that neighbouring rows share a class."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(64, 19, generator=torch.Generator().manual_seed(0)))

    def forward(self, x):
        block = (torch.floor(x[:, 0, :] * 8).long() * 5 + torch.floor(x[:, 1, :] * 8).long()) % 64
        return torch.log_softmax(self.w[block], -1)


def test_label_scan_with_instances(dev, monkeypatch, tmp_path):
    g9, g = golden("g9_kitti.npz"), golden("g18_kitti_view.npz")
    lmap = {int(k): int(v) for k, v in zip(g9["map_keys"], g9["map_values"])}
    raw, words = np.ascontiguousarray(g9["bin"]), np.ascontiguousarray(g9["label"])
    M, n = len(raw), 4096
    seg = V.FrameSegmenter(Stub().to(dev), V.Calibration(g["R"], g["T"], g["P"]), g["colors"], npoints=n)
    sf = kitti.ScanFilter(lmap, "all", device=dev)
    lut = torch.arange(100, 119, dtype=torch.int32, device=dev)
    raw_d, words_d = torch.from_numpy(raw).to(dev), torch.from_numpy(words.view(np.int32)).to(dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(5)
    # instances=None is today's call, key for key
    a = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=gen(), lut=lut)
    keep = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
    b = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=gen(), lut=lut, instances=None)
    assert set(b) == set(keep)
    for k, v in keep.items():
        assert (b[k] is None and v is None) or torch.equal(b[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
    spec = V.InstanceSpec(0.5, range(8), connectivity=26, min_points=3)
    out = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=gen(), lut=lut, instances=spec)
    torch.cuda.synchronize()
    assert set(out) == set(keep) | {"scan_instances", "instance_count", "kept_classes", "kept_instances"}
    assert torch.equal(out["scan_labels"], keep["scan_labels"])      # the low halves are what they were
    assert int(seg.error_flag.item()) == 0 and int(seg._raw_state["instances"]["grid"].error_flag.item()) == 0
    count = int(out["count"].item())
    index = out["index"][:count].cpu().numpy()
    classes = out["kept_classes"][:count].cpu().numpy()
    kept = SR.scan_filter(raw, words, SR.make_lut(lmap))
    assert np.array_equal(index, kept["index"]) and classes.min() >= -1 and classes.max() < 19
    # the classes ARE label_scan's own: where a row has a voter, lut[class] is its scan label
    voted = classes >= 0
    scan_labels = keep["scan_labels"].cpu().numpy()
    assert voted.any() and np.array_equal(scan_labels[index][voted], 100 + classes[voted]) and not scan_labels[index][~voted].any()
    grid, vox_labels = mode_grid(kept["points"], classes, 0.5)
    ref = R.cluster(kept["points"], 0.0, 0.5, vox_labels, classes, grid=grid, member=[1] * 8, min_points=3)
    want = np.zeros(M, np.int32)
    want[index] = ref["row_component"] + 1
    got = out["scan_instances"].cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (M,) and np.array_equal(got, want)
    assert int(out["instance_count"].item()) == ref["count"] > 5 and (want == 0).any() and want.max() == ref["count"]
    assert np.array_equal(out["kept_instances"][:count].cpu().numpy(), ref["row_component"])
    assert set(classes[ref["row_component"] >= 0].tolist()) <= set(range(8))

    # nothing is read back on the way, and the same bytes again
    def forbidden(*args, **kwargs):
        raise AssertionError("label_scan read something back")
    with monkeypatch.context() as mp:
        for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "nonzero"):
            mp.setattr(torch.Tensor, name, forbidden)
        mp.setattr(torch.cuda, "synchronize", forbidden)
        again = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=gen(), lut=lut, instances=spec)
    torch.cuda.synchronize()
    assert again["scan_instances"].cpu().numpy().tobytes() == got.tobytes()
    fn, plain = str(tmp_path / "000000.label"), str(tmp_path / "plain.label")
    kitti.write_labels(fn, again["scan_labels"], again["scan_instances"])
    kitti.write_labels(plain, keep["scan_labels"])
    both = np.fromfile(fn, np.uint32)
    assert np.array_equal(both >> 16, want) and np.array_equal(both & 0xFFFF, np.fromfile(plain, np.uint32))
