"""GPU: voxel-grid downsampling (``pn2_voxel_grid``, csrc/voxel.hip; ``voxel.VoxelGrid``) against the numpy statement of its rule
(tests/voxel_ref.py), exactly -- integers and float bits -- and through ``FrameSegmenter.frame_raw(voxel=)`` and
``load_scans(ingest="device", voxel=)``.  Every ABI call runs with poisoned outputs and a 0xEE-filled workspace (``run_abi``):
every byte outside ``[out_begin[b], out_begin[b] + count[b])``, and every ``inverse`` entry outside the clouds' rows, must come
back untouched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scan_filter_ref as SR
import voxel_ref as R
from conftest import golden
from pointnet12_amd import _lib, kitti, voxel
from pointnet12_amd import kitti_view as V

pytestmark = pytest.mark.gpu

T = _lib.VOXEL_TILE
POISON_F, POISON_I = 0x5A5A5A5A, -777
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 131071, 128 * T + 1]     # (129 tiles: the scan's carry takes a third step)
ALL_OUTPUTS = ("points", "labels", "index", "inverse", "n_points")


def run_abi(dev, pts, labels, begins, counts, max_rows, origin, vox, out_begins=None, out_rows=None, want=ALL_OUTPUTS,
            in_offset=0, out_offset=0):
    """One ``pn2_voxel_grid`` call on host arrays.  Poisons every output, fills the workspace with 0xEE, checks that nothing outside
    the written ranges changed and returns ``(per-cloud dicts, counts, err)`` as numpy; an output not in ``want`` is passed as
    NULL.  ``in_offset`` / ``out_offset``: floats by which ``pts`` / ``out_points`` are shifted off their 16-byte alignment."""
    lib = _lib.load()
    pts = np.ascontiguousarray(pts, np.float32)
    rows, ld = pts.shape
    B = len(begins)
    out_begins = list(begins) if out_begins is None else list(out_begins)
    out_rows = rows if out_rows is None else out_rows
    flat = torch.zeros(rows * ld + in_offset, dtype=torch.float32, device=dev)
    flat[in_offset:].copy_(torch.from_numpy(pts.reshape(-1)))
    lab_d = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
    t64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)
    begin_d, count_d, ob_d = t64(begins), t64(counts), t64(out_begins)
    o_pts = torch.full((out_rows * ld + out_offset,), POISON_F, dtype=torch.int32, device=dev)
    o_lab, o_idx, o_pop = (torch.full((out_rows,), POISON_I, dtype=torch.int32, device=dev) for _ in range(3))
    o_inv = torch.full((rows,), POISON_I, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -5, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = lib.pn2_voxel_grid_workspace_bytes(B, max_rows)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    org_a, vox_a = np.ascontiguousarray(R.triple(origin)), np.ascontiguousarray(R.triple(vox))
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p = _lib.ptr
    opt = lambda name, t: p(t) if name in want else None
    rc = lib.pn2_voxel_grid(flat.data_ptr() + 4 * in_offset, ld, p(lab_d), p(begin_d), p(count_d), B, max_rows, dp(org_a), dp(vox_a),
                            p(ob_d), (o_pts.data_ptr() + 4 * out_offset) if "points" in want else None, opt("labels", o_lab),
                            opt("index", o_idx), p(cnt), opt("inverse", o_inv), opt("n_points", o_pop), p(err), p(ws), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    pts_h = o_pts.cpu().numpy()
    assert (pts_h[:out_offset] == POISON_F).all()
    pts_h = pts_h[out_offset:].reshape(out_rows, ld)
    lab_h, idx_h, pop_h, inv_h, cnt_h = o_lab.cpu().numpy(), o_idx.cpu().numpy(), o_pop.cpu().numpy(), o_inv.cpu().numpy(), cnt.cpu().numpy()
    written, seen = np.zeros(out_rows, bool), np.zeros(rows, bool)
    clouds = []
    for b in range(B):
        looked = max(0, min(counts[b], max_rows))
        lo, hi = out_begins[b], out_begins[b] + int(cnt_h[b])
        assert 0 <= cnt_h[b] <= looked and hi <= out_rows and not written[lo:hi].any()
        written[lo:hi] = True
        seen[begins[b]:begins[b] + looked] = True
        clouds.append({"points": pts_h[lo:hi].view(np.float32), "labels": lab_h[lo:hi], "index": idx_h[lo:hi], "n_points": pop_h[lo:hi],
                       "inverse": inv_h[begins[b]:begins[b] + looked], "count": int(cnt_h[b])})
    for name, arr in (("points", pts_h.view(np.uint32)), ("labels", lab_h), ("index", idx_h), ("n_points", pop_h)):
        poison = POISON_F if name == "points" else POISON_I
        assert (arr[~written] == poison).all() if name in want else (arr == poison).all(), "%s written outside the voxel ranges" % name
    assert (inv_h[~seen] == POISON_I).all() if "inverse" in want else (inv_h == POISON_I).all(), "inverse written outside the clouds"
    return clouds, cnt_h, int(err.item())


def compare(ref, got, want=ALL_OUTPUTS, labelled=True):
    """One cloud's device result against ``voxel_ref.voxel_grid``'s dict: exact, on integers and float bits."""
    assert got["count"] == ref["count"]
    if "points" in want:
        assert np.array_equal(got["points"].view(np.uint32), ref["points"].view(np.uint32))
    if "labels" in want:
        assert np.array_equal(got["labels"], ref["labels"] if labelled else np.zeros(ref["count"], np.int32))
    for name in ("index", "inverse", "n_points"):
        if name in want:
            assert np.array_equal(got[name], ref[name]), name


def run_and_compare(dev, pts, labels, origin, vox, max_rows=None, **kw):
    """One cloud through ``run_abi`` and ``compare``; returns ``(ref, got, err)``."""
    M = len(pts)
    ref = R.voxel_grid(pts, origin, vox, labels)
    clouds, cnt, err = run_abi(dev, pts, labels, [0], [M], M if max_rows is None else max_rows, origin, vox, **kw)
    compare(ref, clouds[0], kw.get("want", ALL_OUTPUTS), labels is not None)
    return ref, clouds[0], err


def random_rows(rng, M, vox, per_voxel=4.0, ld=4):
    """Rows in a cube of about ``M / per_voxel`` cells that straddles the origin."""
    side = max(1.0, (M / per_voxel) ** (1.0 / 3.0)) * vox
    pts = rng.normal(size=(M, ld)).astype(np.float32)
    pts[:, :3] = rng.uniform(-0.4 * side, 0.6 * side, size=(M, 3)).astype(np.float32)
    return pts


def lattice_rows(rng, M, ld=4):
    """Every row in a unit cell of its own: a shuffled integer lattice around the origin, somewhere inside each cell."""
    i = rng.permutation(M)
    cell = np.stack([i % 61 - 30, (i // 61) % 59 - 29, i // (61 * 59) - 18], 1)
    pts = rng.normal(size=(M, ld)).astype(np.float32)
    pts[:, :3] = (cell + rng.uniform(0.1, 0.9, size=(M, 3))).astype(np.float32)
    return pts


@pytest.mark.parametrize("M", SIZES)
def test_sizes_and_patterns(dev, M):
    rng = np.random.default_rng(M)
    labels = rng.integers(0, 19, M).astype(np.int32)
    # about four rows per voxel
    pts = random_rows(rng, M, 0.1)
    ref, got, err = run_and_compare(dev, pts, labels, 0.0, 0.1)
    assert err == 0 and (M < 1000 or 0.15 * M < ref["count"] < 0.6 * M)
    # ALL rows in one voxel: one slot takes every compare-and-swap, minimum and add
    one = rng.normal(size=(M, 4)).astype(np.float32)
    one[:, :3] = rng.uniform(0.01, 0.09, size=(M, 3)).astype(np.float32)
    ref, got, err = run_and_compare(dev, one, labels, 0.0, 0.1)
    assert err == 0 and got["count"] == 1 and got["n_points"].tolist() == [M] and not got["inverse"].any() and got["index"].tolist() == [0]
    # every row in a voxel of its own, max_rows = M: the table at its highest load, probe chains are certain
    lat = lattice_rows(rng, M)
    ref, got, err = run_and_compare(dev, lat, labels, 0.0, 1.0, max_rows=M)
    assert err == 0 and got["count"] == M and np.array_equal(got["index"], np.arange(M)) and (got["n_points"] == 1).all()
    assert np.array_equal(got["inverse"], np.arange(M))


def test_cells_that_differ_in_high_bits_or_sign(dev):
    """Packing and bias mistakes: (+-k * 2^10, 0, 0) and the same on y and z share every low bit; the corner cells are valid."""
    rng = np.random.default_rng(3)
    k = np.arange(1, 1024, dtype=np.float64) * 1024.0
    rows = [np.zeros((1, 3))]
    for a in range(3):
        for sign in (1.0, -1.0):
            block = np.zeros((len(k), 3))
            block[:, a] = sign * k
            rows.append(block)
    for a in range(3):                                               # the corners -2^20 and 2^20 - 1
        for v in (-1048576.0, 1048575.0):
            c = np.zeros((1, 3))
            c[0, a] = v
            rows.append(c)
    rows.append(np.array([[-1048576.0] * 3, [1048575.0] * 3, [-1048576.0, 1048575.0, -1048576.0]]))
    cells = np.concatenate(rows, 0)
    cells = np.concatenate([cells, cells[rng.permutation(len(cells))]], 0)          # every cell twice, the second time shuffled
    pts = np.concatenate([cells + rng.uniform(0.0, 0.5, size=cells.shape), rng.normal(size=(len(cells), 1))], 1).astype(np.float32)
    assert np.array_equal(np.floor(pts[:, :3].astype(np.float64)), cells)            # (float32 holds 2^20 + 0.5 exactly enough)
    ref, got, err = run_and_compare(dev, pts, np.arange(len(pts), dtype=np.int32), 0.0, 1.0)
    assert err == 0 and ref["valid"].all() and got["count"] == len(cells) // 2 and (got["n_points"] == 2).all()
    assert np.array_equal(got["index"], np.arange(len(cells) // 2))


def test_rows_outside_the_grid_are_dropped(dev):
    inf, nan = np.inf, np.nan
    bad = []
    for a in range(3):
        for v in (-1048577.0, 1048576.0, 1e30, -1e30, nan, inf, -inf):
            r = [0.5, 0.5, 0.5, 1.0]
            r[a] = v
            bad.append(r)
    good = [[0.5, 0.5, 0.5, 2.0], [-1048576.0, 0.5, 0.5, 3.0], [1048575.5, 0.5, 0.5, 4.0], [0.5, 0.5, 0.75, nan]]
    pts = np.array(bad[:5] + good[:2] + bad[5:] + good[2:], np.float32)   # invalid rows first: they must not take a rank
    ref, got, err = run_and_compare(dev, pts, np.arange(len(pts), dtype=np.int32), 0.0, 1.0)
    assert err == _lib.VOXEL_ERR_RANGE and ref["valid"].sum() == 4 and got["count"] == 3
    assert (got["inverse"][~ref["valid"]] == -1).all() and got["index"].tolist() == [5, 6, len(pts) - 2]
    assert got["n_points"].tolist() == [2, 1, 1]                     # (a NaN in column 3 is no coordinate)
    # all rows invalid: an empty result, nothing written
    ref, got, err = run_and_compare(dev, np.array(bad, np.float32), None, 0.0, 1.0)
    assert err == _lib.VOXEL_ERR_RANGE and got["count"] == 0 and (got["inverse"] == -1).all()


def test_planted_border_values_and_an_anisotropic_grid(dev):
    x = [np.float32(0.1), np.float32(0.3), -0.05, -0.0, 0.0, np.float32(0.7), np.float32(-0.1), np.float32(-0.3)]
    pts = np.zeros((len(x), 4), np.float32)
    pts[:, 0] = x
    ref, got, err = run_and_compare(dev, pts, None, 0.0, 0.1)
    q, _ = R.cells(pts, 0.0, 0.1)
    assert err == 0 and q[:5, 0].tolist() == [1.0, 3.0, -1.0, 0.0, 0.0] and got["inverse"][3] == got["inverse"][4]
    m = np.arange(-40, 41, dtype=np.float32) * np.float32(0.125)     # exact multiples of the voxel size, on every axis in turn
    for a in range(3):
        pts = np.zeros((len(m), 4), np.float32)
        pts[:, a] = m
        ref, got, err = run_and_compare(dev, pts, None, 0.0, 0.125)
        assert err == 0 and got["count"] == len(m)
    rng = np.random.default_rng(11)
    pts = rng.normal(scale=3.0, size=(5000, 4)).astype(np.float32)
    ref, got, err = run_and_compare(dev, pts, rng.integers(0, 5, 5000).astype(np.int32), (0.25, -3.0, 1e-3), (0.3, 0.7, 1.1))
    assert err == 0 and 500 < got["count"] < 4000


def test_batched_clouds_with_identical_coordinates_do_not_merge(dev):
    rng = np.random.default_rng(5)
    base = random_rows(rng, T + 5, 0.1)
    counts = [T + 5, 0, 200]
    begins = [3, T + 20, T + 20]
    rows = T + 20 + 200 + 9
    pts = rng.normal(size=(rows, 4)).astype(np.float32)
    labels = rng.integers(0, 19, rows).astype(np.int32)
    for b, c in zip(begins, counts):
        pts[b:b + c] = base[:c]                                      # the SAME coordinates in every cloud
    out_begins = [11, 5, T + 40]
    out_rows = T + 40 + 200 + 3
    refs = [R.voxel_grid(pts[b:b + c], 0.0, 0.1, labels[b:b + c]) for b, c in zip(begins, counts)]
    clouds, cnt, err = run_abi(dev, pts, labels, begins, counts, T + 5, 0.0, 0.1, out_begins, out_rows)
    assert err == 0 and cnt.tolist() == [r["count"] for r in refs] and cnt[1] == 0 and cnt[2] > 50
    for b in range(3):
        compare(refs[b], clouds[b])
    # a row_count above max_rows: its bit is set and the rows beyond max_rows are ignored
    short = R.voxel_grid(pts[3:3 + T], 0.0, 0.1, labels[3:3 + T])
    clouds, cnt, err = run_abi(dev, pts, labels, begins, counts, T, 0.0, 0.1, out_begins, out_rows)
    assert err == _lib.VOXEL_ERR_ROWS and cnt.tolist() == [short["count"], 0, refs[2]["count"]]
    compare(short, clouds[0])
    compare(refs[2], clouds[2])
    # through the class: outputs at row_begin, check() raises
    vg = voxel.VoxelGrid(0.1, device=dev)
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    p, l, i, c, inv, pop = vg.downsample(torch.from_numpy(pts).to(dev), torch.from_numpy(labels).to(dev), t64(begins), t64(counts), T + 5)
    vg.check()
    c = c.cpu().tolist()
    assert c == [r["count"] for r in refs]
    for b in (0, 2):
        lo, hi = begins[b], begins[b] + c[b]
        got = {"points": p[lo:hi].cpu().numpy(), "labels": l[lo:hi].cpu().numpy(), "index": i[lo:hi].cpu().numpy(),
               "n_points": pop[lo:hi].cpu().numpy(), "inverse": inv[begins[b]:begins[b] + counts[b]].cpu().numpy(), "count": c[b]}
        compare(refs[b], got)
    vg.downsample(torch.from_numpy(pts).to(dev), None, t64(begins), t64(counts), T)
    with pytest.raises(ValueError):
        vg.check()
    # the [B, M, ld] form: row_begin / row_count default to the obvious values
    cube = np.ascontiguousarray(np.stack([base[:700], base[:700], base[300:1000]], 0))
    p, l, i, c, inv, pop = vg.downsample(torch.from_numpy(cube).to(dev))
    assert l is None
    for b in range(3):
        ref = R.voxel_grid(cube[b], 0.0, 0.1)
        m = int(c[b].item())
        got = {"points": p[b * 700:b * 700 + m].cpu().numpy(), "index": i[b * 700:b * 700 + m].cpu().numpy(),
               "n_points": pop[b * 700:b * 700 + m].cpu().numpy(), "inverse": inv[b * 700:(b + 1) * 700].cpu().numpy(), "count": m}
        compare(ref, got, ("points", "index", "inverse", "n_points"))


@pytest.mark.parametrize("ld,in_offset,out_offset", [(3, 0, 0), (4, 0, 0), (4, 1, 0), (4, 0, 1), (4, 1, 1), (7, 0, 0), (16, 0, 0)])
def test_row_widths_alignment_and_optional_outputs(dev, ld, in_offset, out_offset):
    rng = np.random.default_rng(ld * 10 + in_offset)
    M = 2 * T + 77
    pts = random_rows(rng, M, 0.25, ld=ld)
    pts[17, 1] = np.nan                                              # one dropped row
    labels = rng.integers(0, 19, M).astype(np.int32)
    ref, got, err = run_and_compare(dev, pts, labels, 0.0, 0.25, in_offset=in_offset, out_offset=out_offset)
    assert err == _lib.VOXEL_ERR_RANGE and got["inverse"][17] == -1
    run_and_compare(dev, pts, None, 0.0, 0.25, in_offset=in_offset, out_offset=out_offset)       # labels absent: zeros
    if in_offset == out_offset:
        for missing in ALL_OUTPUTS:                                  # each optional output NULL in turn
            run_and_compare(dev, pts, labels, 0.0, 0.25, in_offset=in_offset, out_offset=out_offset,
                            want=tuple(n for n in ALL_OUTPUTS if n != missing))
        run_and_compare(dev, pts, labels, 0.0, 0.25, want=())        # the count alone


def test_same_result_whatever_the_order_or_schedule(dev):
    rng = np.random.default_rng(9)
    M = 50000
    pts = random_rows(rng, M, 0.1)
    runs = [run_abi(dev, pts, None, [0], [M], M, 0.0, 0.1)[0][0] for _ in range(2)]
    for name in ("points", "index", "inverse", "n_points"):
        assert np.array_equal(runs[0][name].view(np.uint32), runs[1][name].view(np.uint32)), name
    back = run_abi(dev, pts[::-1], None, [0], [M], M, 0.0, 0.1)[0][0]
    assert back["count"] == runs[0]["count"]
    # the same voxels with the same populations: compared by key, since the reversed run keeps each voxel's LAST row
    key = lambda p: R.keys(p, 0.0, 0.1)[0]
    a, b = np.argsort(key(runs[0]["points"])), np.argsort(key(back["points"]))
    assert np.array_equal(key(runs[0]["points"])[a], key(back["points"])[b]) and np.array_equal(runs[0]["n_points"][a], back["n_points"][b])
    # mapped back: row i of the forward run is row M - 1 - i of the reversed one, and both lie in the same voxel
    fwd_voxel = key(runs[0]["points"])[runs[0]["inverse"]]
    back_voxel = key(back["points"])[back["inverse"][::-1]]
    assert np.array_equal(fwd_voxel, back_voxel)
    # the representative's coordinates: the forward run's are the voxel's lowest row, which is what the reference says
    compare(R.voxel_grid(pts, 0.0, 0.1), runs[0], ("points", "index", "inverse", "n_points"))
    compare(R.voxel_grid(pts[::-1], 0.0, 0.1), back, ("points", "index", "inverse", "n_points"))


@pytest.mark.parametrize("size,count", [(0.1, 4800), (0.05, 5133), (0.2, 4116), (0.5, 3105)])
def test_recorded_scan(dev, size, count):
    raw = np.ascontiguousarray(golden("g9_kitti.npz")["bin"])
    ref, got, err = run_and_compare(dev, raw, None, 0.0, size)
    assert err == 0 and got["count"] == count and (size != 0.1 or got["n_points"].max() <= 10)


def test_capture_and_replay_with_other_rows_and_count(dev):
    rng = np.random.default_rng(21)
    cap = 3 * T + 17
    cloud_a, cloud_b = random_rows(rng, cap, 0.1), random_rows(rng, 2 * T + 3, 0.1)
    lab_a, lab_b = (rng.integers(0, 19, len(c)).astype(np.int32) for c in (cloud_a, cloud_b))
    vg = voxel.VoxelGrid(0.1, device=dev)
    bufs = vg.buffers(cap)
    pts_s = torch.zeros(cap, 4, device=dev)
    lab_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    begin = torch.zeros(1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def load(cloud, lab):
        pts_s[:len(cloud)].copy_(torch.from_numpy(cloud))
        lab_s[:len(cloud)].copy_(torch.from_numpy(lab))
        count.fill_(len(cloud))

    def step():
        return vg.downsample(pts_s, lab_s, begin, count, cap, out=bufs)

    def snapshot():
        torch.cuda.synchronize()
        m, rows = int(bufs.count.item()), int(count.item())
        return {"points": bufs.points[:m].cpu().numpy(), "labels": bufs.labels[:m].cpu().numpy(), "index": bufs.index[:m].cpu().numpy(),
                "n_points": bufs.n_points[:m].cpu().numpy(), "inverse": bufs.inverse[:rows].cpu().numpy(), "count": m}

    load(cloud_a, lab_a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for cloud, lab in ((cloud_b, lab_b), (cloud_a, lab_a), (cloud_b[:T - 1], lab_b[:T - 1])):
        load(cloud, lab)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before               # nothing allocated by a replay
        replayed = snapshot()
        bufs.count.zero_()
        bufs.inverse.fill_(POISON_I)
        step()
        eager = snapshot()
        ref = R.voxel_grid(cloud, 0.0, 0.1, lab)
        compare(ref, replayed)
        compare(ref, eager)
        assert int(vg.error_flag.item()) == 0


class Stub(torch.nn.Module):
    """A tiny stand-in for the network: ``[1, 4, n]`` -> log-probabilities ``[1, n, 19]``."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(4, 19, generator=torch.Generator().manual_seed(0)))

    def forward(self, x):
        return torch.log_softmax(x.transpose(2, 1) @ self.w, -1)


def test_frame_raw_with_a_voxel_grid(dev):
    g9, g = golden("g9_kitti.npz"), golden("g18_kitti_view.npz")
    lmap = {int(k): int(v) for k, v in zip(g9["map_keys"], g9["map_values"])}
    raw, words = np.ascontiguousarray(g9["bin"]), np.ascontiguousarray(g9["label"])
    n = 4096
    seg = V.FrameSegmenter(Stub().to(dev), V.Calibration(g["R"], g["T"], g["P"]), g["colors"], npoints=n)
    sf = kitti.ScanFilter(lmap, "all", device=dev)
    vg = voxel.VoxelGrid(0.2, device=dev)
    # what the filter keeps (subset "all": the class drop only, no angle is compared), then the rule on those rows
    kept = SR.scan_filter(raw, words, SR.make_lut(lmap))
    ref = R.voxel_grid(kept["points"], 0.0, 0.2)
    count = ref["count"]
    assert 0 < count <= n < len(kept["points"])                      # every representative is drawn at least once
    out = seg.frame_raw(raw, words, scan_filter=sf, rng="cover", voxel=vg)
    assert int(seg.error_flag.item()) == 0 and int(sf.error_flag.item()) == 0 and int(vg.error_flag.item()) == 0
    assert int(out["voxel_count"].item()) == count and int(out["count"].item()) == len(kept["points"])
    drawn = np.arange(n) % count
    assert np.array_equal(out["pts_3d"].cpu().numpy().view(np.uint32), ref["points"][drawn][:, :3].view(np.uint32))
    assert np.array_equal(out["voxel_index"][:count].cpu().numpy(), kept["index"][ref["index"]])
    assert np.array_equal(raw[out["voxel_index"][:count].cpu().numpy()].view(np.uint32), ref["points"].view(np.uint32))
    inverse = out["voxel_inverse"][:len(kept["points"])]
    assert np.array_equal(inverse.cpu().numpy(), ref["inverse"])
    # every kept row takes the prediction of its representative: the first `count` draws ARE the representatives, in order
    pred_of_reps = out["pred"][:count]
    spread = voxel.expand(pred_of_reps, inverse, -1)
    assert np.array_equal(spread.cpu().numpy(), out["pred"].cpu().numpy()[:count][ref["inverse"]])
    assert voxel.expand(pred_of_reps, torch.tensor([0, -1, count - 1], device=dev), -9).tolist() == \
        [int(pred_of_reps[0]), -9, int(pred_of_reps[count - 1])]
    two = voxel.expand(out["log_probs"][:count], inverse, 0.0)       # rows of a matrix
    assert torch.equal(two, out["log_probs"][:count][inverse.long()])
    # rng="numpy" draws from the voxel count
    np.random.seed(4)
    b = seg.frame_raw(raw, words, scan_filter=sf, voxel=vg)
    np.random.seed(4)
    expect = ref["points"][np.random.choice(count, n, replace=True)]
    assert np.array_equal(b["pts_3d"].cpu().numpy().view(np.uint32), expect[:, :3].view(np.uint32))
    # voxel=None is today's path, bit for bit; "cover" without a grid walks the kept rows
    choice = np.random.default_rng(5).integers(0, len(kept["points"]), n)
    a = seg.frame_raw(raw, words, scan_filter=sf, choice=choice)
    keep = {k: a[k].clone() for k in ("image", "pred", "top_view", "pts_2d", "points", "log_probs")}
    b = seg.frame_raw(raw, words, scan_filter=sf, choice=choice, voxel=None)
    assert set(a) == set(b) and "voxel_count" not in b
    assert all(torch.equal(keep[k].view(torch.uint8), b[k].contiguous().view(torch.uint8)) for k in keep)
    c = seg.frame_raw(raw, words, scan_filter=sf, rng="cover")
    assert np.array_equal(c["pts_3d"].cpu().numpy().view(np.uint32), kept["points"][np.arange(n) % len(kept["points"])][:, :3].view(np.uint32))
    # label_scan with a grid: the queries remain ALL kept rows, so every kept row gets a label
    d = seg.label_scan(raw, words, scan_filter=sf, rng="cover", voxel=vg, max_dist=None)
    labelled = np.zeros(len(raw), bool)
    labelled[kept["index"]] = True
    scan_labels = d["scan_labels"].cpu().numpy()
    assert scan_labels.shape == (len(raw),) and not scan_labels[~labelled].any() and int(d["voxel_count"].item()) == count


def test_load_scans_device_ingest_with_a_voxel_grid(dev, tmp_path):
    g9 = golden("g9_kitti.npz")
    lmap = {int(k): int(v) for k, v in zip(g9["map_keys"], g9["map_values"])}
    raw, words = SR.decided_scan(31, 8000, classes=sorted(lmap))
    pairs, at = [], 0
    for k, m in enumerate((T + 7, 0, 3000, 517)):
        fv, fl = os.path.join(tmp_path, "%06d.bin" % k), os.path.join(tmp_path, "%06d.label" % k)
        raw[at:at + m].tofile(fv)
        words[at:at + m].tofile(fl)
        pairs.append((fv, fl))
        at += m
    vg = voxel.VoxelGrid(8.0, device=dev)                            # (the decided scans spread over +-60 m: coarse cells, so that rows merge)
    for subset in ("inview", "all"):
        refs = []
        for fv, fl in pairs:
            p, l = kitti.read_scan(fv, fl, lmap, subset)
            refs.append(R.voxel_grid(p, 0.0, 8.0, l))
        want_p = np.concatenate([r["points"] for r in refs], 0)
        want_l = np.concatenate([r["labels"] for r in refs], 0)
        assert 0 < len(want_p) < sum(len(kitti.read_scan(fv, fl, lmap, subset)[0]) for fv, fl in pairs)
        for chunk_rows in (1 << 22, 2000):                           # one chunk; three chunks
            store = kitti.load_scans(pairs, lmap, subset, device=dev, ingest="device", chunk_rows=chunk_rows, voxel=vg)
            assert store.row_count.tolist() == [r["count"] for r in refs]
            assert np.array_equal(store.raw.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
            assert np.array_equal(store.label.cpu().numpy(), want_l) and store.label.dtype == torch.int32
    with pytest.raises(ValueError):
        kitti.load_scans(pairs, lmap, voxel=vg)                      # a grid needs the device ingest
