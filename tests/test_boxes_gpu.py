"""GPU: ``pn2_segment_boxes`` (csrc/boxes.hip) and what is built on it (``boxes.segment_boxes`` / ``instance_boxes``,
``kitti_view.InstanceSpec(boxes=True)``) against the numpy statement of the rule (tests/box_ref.py): RAW BITS throughout, no tolerance
anywhere.  Every ABI call runs with poisoned outputs and a 0xEE-filled workspace; every byte outside the written ranges must come back
untouched."""
import math

import numpy as np
import pytest
import torch

import box_ref as R
import scan_filter_ref as SR
from conftest import golden
from pointnet12_amd import _lib, boxes, kitti, plane, voxel
from pointnet12_amd import kitti_view as V

pytestmark = pytest.mark.gpu

POISON_F, POISON_I, POISON_L = 0x5A5A5A5A, -777, -(1 << 40) - 5
FLOATS = {"center": 3, "size": 3, "yaw": 1, "lo": 3, "hi": 3}
NAMES = ("center", "size", "yaw", "angle", "lo", "hi", "n", "score")
SPLIT = 256                                                          # split_rows of most calls here: both sweeps run on small inputs


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def t64(dev, v):
    return torch.tensor([int(x) for x in v], dtype=torch.int64, device=dev)


def written_rows(out_rows, out_begins, out_counts, max_rows):
    written = np.zeros(out_rows, bool)
    for ob, oc in zip(out_begins, out_counts):
        m = max(0, min(int(oc), max_rows))
        assert ob + m <= out_rows and not written[ob:ob + m].any()
        written[ob:ob + m] = True
    return written


class Call:
    """One ``pn2_segment_boxes`` call on host arrays: device inputs, poisoned outputs, a 0xEE workspace and the argument list."""

    def __init__(self, dev, pts, seg, begins, counts, max_rows, out_counts, out_begins=None, out_rows=None, A=64, d0=0.05, axes=(0, 1, 2),
                 split=SPLIT, want=NAMES, in_offset=0, table=None):
        pts = np.ascontiguousarray(pts, np.float32)
        self.rows, self.ld = pts.shape
        self.B, self.max_rows, self.want = len(begins), max_rows, want
        self.out_begins = list(begins) if out_begins is None else list(out_begins)
        self.out_counts, self.out_rows = list(out_counts), self.rows if out_rows is None else out_rows
        self.table_h = R.angle_table(A) if table is None else np.ascontiguousarray(table, np.float32)
        self.flat = torch.zeros(self.rows * self.ld + in_offset, dtype=torch.float32, device=dev)
        self.flat[in_offset:].copy_(torch.from_numpy(pts.reshape(-1)))
        self.pts_ptr = self.flat.data_ptr() + 4 * in_offset
        self.seg = torch.from_numpy(np.ascontiguousarray(seg, np.int32)).to(dev)
        self.begin, self.count = t64(dev, begins), t64(dev, counts)
        self.ob, self.oc = t64(dev, self.out_begins), t64(dev, out_counts)
        self.table = torch.from_numpy(self.table_h).to(dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = {name: torch.full((self.out_rows * w,), POISON_F, dtype=torch.int32, device=dev) for name, w in FLOATS.items()}
        self.out["angle"] = torch.full((self.out_rows,), POISON_I, dtype=torch.int32, device=dev)
        self.out["n"] = torch.full((self.out_rows,), POISON_I, dtype=torch.int32, device=dev)
        self.out["score"] = torch.full((self.out_rows,), POISON_L, dtype=torch.int64, device=dev)
        nbytes = _lib.load().pn2_segment_boxes_workspace_bytes(self.B, max_rows)
        assert nbytes > 0
        self.ws = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
        p, o = _lib.ptr, {k: (v if k in want else None) for k, v in self.out.items()}
        self.args = {"pts": self.pts_ptr, "ld": self.ld, "cx": axes[0], "cy": axes[1], "cz": axes[2], "seg": p(self.seg), "row_begin": p(self.begin),
                     "row_count": p(self.count), "B": self.B, "max_rows": max_rows, "out_begin": p(self.ob), "out_count": p(self.oc),
                     "angles": p(self.table), "A": len(self.table_h), "d0": d0, "split_rows": split, "center": p(o["center"]), "size": p(o["size"]),
                     "yaw": p(o["yaw"]), "angle": p(o["angle"]), "lo": p(o["lo"]), "hi": p(o["hi"]), "n": p(o["n"]), "score": p(o["score"]),
                     "err": p(self.err), "workspace": p(self.ws), "stream": None}

    def launch(self, **changed):
        args = dict(self.args, stream=_lib.stream())
        args.update(changed)
        rc = _lib.load().pn2_segment_boxes(*args.values())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all((v == (POISON_L if k == "score" else POISON_I if k in ("angle", "n") else POISON_F)).all().item() for k, v in self.out.items())

    def result(self):
        """The outputs as numpy (floats as uint32 bits) after checking that nothing outside the written rows changed."""
        written = written_rows(self.out_rows, self.out_begins, self.out_counts, self.max_rows)
        got = {}
        for name, t in self.out.items():
            h = t.cpu().numpy()
            poison = POISON_L if name == "score" else POISON_I if name in ("angle", "n") else POISON_F
            h = h.reshape(self.out_rows, -1)
            assert (h == poison).all() if name not in self.want else (h[~written] == poison).all(), "%s written outside its rows" % name
            got[name] = h.view(np.uint32) if name in FLOATS else h[:, 0]
            if name == "yaw":
                got[name] = got[name][:, 0]
        return got, int(self.err.item())


def check(dev, pts, seg, begins, counts, max_rows, out_counts, **kw):
    """One call against the restatement, cloud by cloud: every output's bits and the error word.  Returns (outputs, err)."""
    call = Call(dev, pts, seg, begins, counts, max_rows, out_counts, **kw)
    assert call.launch() == 0
    got, err = call.result()
    pts, seg = np.ascontiguousarray(pts, np.float32), np.asarray(seg)
    expect_err = 0
    for b in range(len(begins)):
        c, m = max(0, min(int(counts[b]), max_rows)), max(0, min(int(out_counts[b]), max_rows))
        lo, ob = begins[b], call.out_begins[b]
        ref = R.segment_boxes(pts[lo:lo + c], seg[lo:lo + c], m, call.table_h, max(float(kw.get("d0", 0.05)), 0.0), kw.get("axes", (0, 1, 2)))
        expect_err |= ref["err"]
        for name in call.want:
            want = u32(ref[name]) if name in FLOATS else ref[name]
            assert np.array_equal(got[name][ob:ob + m], want), "%s, cloud %d" % (name, b)
    assert err == expect_err
    return got, err


def clusters(rng, populations, ld=3, axes=(0, 1, 2), shuffle=True):
    """One L-shaped cluster per population, each with its own heading and place, in columns ``axes`` of ``ld``; the other columns hold
    noise.  Returns (points, seg)."""
    pts, seg = [], []
    for s, n in enumerate(populations):
        p = R.car_l_shape(rng, n, rng.uniform(0, math.pi / 2), centre=rng.uniform(-30, 30, 2))
        rows = rng.normal(size=(n, ld)).astype(np.float32)
        rows[:, list(axes)] = p
        pts.append(rows)
        seg.append(np.full(n, s, np.int32))
    pts, seg = np.concatenate(pts, 0), np.concatenate(seg)
    order = rng.permutation(len(seg)) if shuffle else np.arange(len(seg))
    return pts[order], seg[order]


POPULATIONS = [0, 1, 2, 63, 64, 65, 129, SPLIT - 1, SPLIT, SPLIT + 1, 3 * SPLIT + 5]


@pytest.mark.parametrize("ld,axes", [(3, (0, 1, 2)), (4, (2, 0, 1)), (6, (3, 5, 4))])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 90, 256])
def test_populations_around_the_wave_and_the_split_threshold(dev, A, ld, axes):
    """Segments of 0, 1, 2, 63, 64, 65, 129 rows and either side of split_rows (lowered to 256): the wave sweep and the workgroup sweep
    in one call; the same call with the library's own threshold (every segment by one wave) gives the same bytes."""
    rng = np.random.default_rng(A * 10 + ld)
    pts, seg = clusters(rng, POPULATIONS, ld, axes)
    seg[rng.choice(np.flatnonzero(seg == len(POPULATIONS) - 1), 20, replace=False)] = -1      # rows that take no part
    N, S = len(seg), len(POPULATIONS)
    got, err = check(dev, pts, seg, [0], [N], N, [S], A=A, axes=axes, out_rows=S + 3)
    assert err == 0 and got["angle"][0] == -1 and (got["angle"][1:S] >= 0).all() and got["n"][:S].sum() == (seg >= 0).sum()
    other, _ = check(dev, pts, seg, [0], [N], N, [S], A=A, axes=axes, out_rows=S + 3, split=0)
    for name in NAMES:
        assert np.array_equal(got[name], other[name]), name
    assert _lib.BOX_SPLIT_ROWS > max(POPULATIONS)                    # (split=0 really took the other path)


def test_three_clouds_device_counts_range_bit_and_null_outputs(dev):
    rng = np.random.default_rng(11)
    pts, seg = clusters(rng, [300, 40, 5, 700, 90], 4)
    N = len(seg)
    tail = rng.normal(size=(12, 4)).astype(np.float32)               # clouds two and three lie behind the first: 2 rows and 0 rows
    pts, seg = np.concatenate([pts, tail], 0), np.concatenate([seg, np.array([1, 0] + [3] * 10, np.int32)])
    begins, counts = [0, N, N + 2], [N, 2, 0]
    out_begins, out_rows = [20, 3, 12], 20 + 5 + 4
    seg[[5, 77]] = -3
    got, err = check(dev, pts, seg, begins, counts, N, [5, 2, 4], out_begins=out_begins, out_rows=out_rows)
    assert err == 0 and got["n"][3:5].tolist() == [1, 1] and (got["angle"][12:16] == -1).all()
    # an out_count below the largest seg: the rows of the segments beyond it take no part, the bit is set, nothing outside is written
    got, err = check(dev, pts, seg, begins, counts, N, [3, 1, 4], out_begins=out_begins, out_rows=out_rows)
    assert err == _lib.BOX_ERR_RANGE
    for value in (5, 6, N - 1, N, 10 ** 6, 2 ** 31 - 1):
        s = seg.copy()
        s[[9, 200]] = value
        _, err = check(dev, pts, s, begins, counts, N, [5, 2, 4], out_begins=out_begins, out_rows=out_rows)
        assert err == _lib.BOX_ERR_RANGE
    # counts above max_rows are clamped; an out_count above it too
    check(dev, pts, seg, begins, [N, 2, 0], 600, [5, 2, 4], out_begins=out_begins, out_rows=out_rows)
    check(dev, pts, seg, [0], [N], N, [10 ** 9], out_rows=N + 4)
    # every optional output NULL in turn, then all of them; a misaligned-by-one-float input
    for name in ("angle", "lo", "hi", "n", "score"):
        check(dev, pts, seg, begins, counts, N, [5, 2, 4], out_begins=out_begins, out_rows=out_rows, want=tuple(k for k in NAMES if k != name))
    check(dev, pts, seg, begins, counts, N, [5, 2, 4], out_begins=out_begins, out_rows=out_rows, want=("center", "size", "yaw"), in_offset=1)
    # err NULL
    call = Call(dev, pts, seg, begins, counts, N, [3, 1, 4], out_begins=out_begins, out_rows=out_rows)
    assert call.launch(err=None) == 0 and call.result()[1] == 0


def disc_rows(scale=1.0, shift=(0.0, 0.0)):
    g = np.arange(-3, 4)
    X, Y = np.meshgrid(g, g)
    m = X ** 2 + Y ** 2 <= 9
    return np.stack([X[m] * scale + shift[0], Y[m] * scale + shift[1], np.zeros(m.sum())], 1).astype(np.float32)


def test_exact_ties_and_special_values(dev):
    rng = np.random.default_rng(13)
    ii, jj = (g.ravel() for g in np.meshgrid(np.arange(40), np.arange(25), indexing="ij"))
    lattice = np.stack([ii, jj, ii % 3], 1).astype(np.float32)       # 1000 rows of integers: exact score and area ties
    same = np.tile(np.array([[3.25, -1.5, 0.75]], np.float32), (300, 1))
    zeros = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]] * 3, np.float32)
    parts = [lattice, disc_rows(), disc_rows(0.5, (7.0, -2.0)), same, zeros, lattice[:70] * np.float32(2.0 ** 40)]
    pts = np.concatenate(parts, 0)
    seg = np.concatenate([np.full(len(p), s, np.int32) for s, p in enumerate(parts)])
    order = rng.permutation(len(seg))
    pts, seg = pts[order], seg[order]
    for A in (64, 256):
        got, err = check(dev, pts, seg, [0], [len(seg)], len(seg), [len(parts)], A=A)
        assert err == 0 and got["angle"][3] == 0 and not got["size"][3].any()          # identical points: every angle ties
    got, _ = check(dev, pts, seg, [0], [len(seg)], len(seg), [len(parts)])
    assert got["angle"][1] == 19                                      # the symmetric disc: 19 and 45 tie, the lowest is returned
    assert (got["lo"][4] == 0x80000000).all() and (got["hi"][4] == 0).all()             # -0.0 < +0.0
    # planted NaN / inf / 2^61 rows, one segment made only of such rows, the largest magnitudes that take part
    bad = pts.copy()
    s = seg.copy()
    at = rng.choice(len(s), 40, replace=False)
    values = [np.nan, np.inf, -np.inf, 2.0 ** 61, -2.0 ** 61]
    for k, row in enumerate(at):
        bad[row, k % 3] = values[k % 5] if not (k % 3 == 2 and k % 5 >= 3) else np.nan    # (a large z takes part: plant a NaN instead)
    extra = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [2.0 ** 61, 0, 0]], np.float32)
    edge = np.array([[2.0 ** 60, -2.0 ** 60, 3e38], [-2.0 ** 60, 2.0 ** 60, -3e38], [1.0, 2.0, 3.0]], np.float32)
    bad = np.concatenate([bad, extra, edge], 0)
    s = np.concatenate([s, np.full(4, len(parts), np.int32), np.full(3, len(parts) + 1, np.int32)])
    got, err = check(dev, bad, s, [0], [len(s)], len(s), [len(parts) + 2])
    assert err == _lib.BOX_ERR_NONFINITE and got["angle"][len(parts)] == -1 and got["n"][len(parts)] == 0 and got["n"][len(parts) + 1] == 3
    # a non-finite row outside every segment sets nothing
    s2 = s.copy()
    s2[np.flatnonzero(~R.takes_part(bad, (0, 1, 2)))] = -1
    _, err = check(dev, bad, s2, [0], [len(s2)], len(s2), [len(parts) + 2])
    assert err == 0


@pytest.mark.parametrize("d0", [0.0, -0.0, -1.0])
def test_a_d0_at_or_below_zero_is_the_area_criterion(dev, d0):
    rng = np.random.default_rng(17)
    pts, seg = clusters(rng, [50, 300, 7], 3)
    got, err = check(dev, pts, seg, [0], [len(seg)], len(seg), [3], d0=d0)
    assert err == 0 and not got["score"][:3].any()
    b = boxes.segment_boxes(torch.from_numpy(pts).to(dev), torch.from_numpy(seg).to(dev), 3, criterion="area", d0=0.3)
    mine = as_numpy(b, 3)
    for name in NAMES:
        assert np.array_equal(mine[name].reshape(3, -1), got[name][:3].reshape(3, -1)), name
    closeness = boxes.segment_boxes(torch.from_numpy(pts).to(dev), torch.from_numpy(seg).to(dev), 3)
    assert (closeness.score[:3] > 0).all() and (closeness.angle[3:] == -1).all() and not closeness.center[3:].any()


def test_refusals_touch_nothing(dev):
    rng = np.random.default_rng(19)
    pts, seg = clusters(rng, [50, 30], 4)
    call = Call(dev, pts, seg, [0], [len(seg)], len(seg), [2])
    a = call.args
    refused = [{k: None} for k in ("pts", "seg", "row_begin", "row_count", "out_begin", "out_count", "angles", "center", "size", "yaw", "workspace")]
    refused += [{"A": 0}, {"A": 257}, {"A": -1}, {"cx": 1}, {"cz": 0}, {"cy": 2}, {"cx": 4}, {"cy": -1}, {"cz": 4}, {"ld": 2}, {"B": 0}, {"B": 65536},
                {"max_rows": -1}, {"max_rows": (1 << 29) + 1}, {"d0": float("nan")}, {"d0": float("inf")}, {"d0": -float("inf")},
                {"split_rows": 63}, {"split_rows": -1}, {"split_rows": (1 << 29) + 1}]
    refused += [{k: a[k] + 2} for k in ("pts", "seg", "center", "size", "yaw", "angle", "lo", "hi", "n", "err")]
    refused += [{"score": a["score"] + 4}, {"angles": a["angles"] + 4}, {"workspace": a["workspace"] + 8}]
    for change in refused:
        assert call.launch(**change) == -1, change
        assert call.untouched() and int(call.err.item()) == 0 and (call.ws == 0xEE).all().item(), change
    assert call.launch() == 0 and not call.untouched()


def as_numpy(b, count):
    return {name: (u32(getattr(b, name)[:count].cpu().numpy()) if name in FLOATS else getattr(b, name)[:count].cpu().numpy()) for name in NAMES}


def same_as_ref(got, pts, seg, count, A=64, d0=0.05):
    ref = R.segment_boxes(pts, seg, count, R.angle_table(A), d0)
    for name in NAMES:
        assert np.array_equal(got[name].reshape(count, -1), (u32(ref[name]) if name in FLOATS else ref[name]).reshape(count, -1)), name
    return ref


def test_two_runs_are_byte_identical_and_a_graph_replays_on_new_inputs(dev):
    rng = np.random.default_rng(23)
    cap = 6000
    scenes = [clusters(rng, [1500, 900, 64, 3, 0, 2000], 4), clusters(rng, [10, 700], 4), clusters(rng, [300] * 17, 4)]
    pts_s = torch.zeros(cap, 4, device=dev)
    inv_s = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    begin = torch.zeros(1, dtype=torch.int64, device=dev)
    rows, segs = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    buf = boxes.buffers(cap, 1, cap, 64, dev)

    def load(scene, count):
        pts_s[:len(scene[0])].copy_(torch.from_numpy(scene[0]))
        inv_s[:len(scene[1])].copy_(torch.from_numpy(scene[1]))
        rows.fill_(len(scene[1]))
        segs.fill_(count)

    def step():
        return boxes.segment_boxes(pts_s, inv_s, segs, row_begin=begin, row_count=rows, max_rows=cap, buffers=buf, split_rows=1024)

    load(scenes[0], 6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = as_numpy(buf.boxes(), 6)
    same_as_ref(first, *scenes[0], 6)
    step()
    torch.cuda.synchronize()
    again = as_numpy(buf.boxes(), 6)
    for name in NAMES:
        assert np.array_equal(first[name], again[name]), name
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for scene, count in ((scenes[1], 2), (scenes[2], 17), (scenes[0], 6), (scenes[2], 9)):
        load(scene, count)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before               # nothing allocated by a replay
        replayed, flag = as_numpy(buf.boxes(), count), int(buf.error_flag.item())
        buf.center.fill_(3.0)
        buf.score.fill_(-1)
        step()
        torch.cuda.synchronize()
        eager = as_numpy(buf.boxes(), count)
        ref = same_as_ref(replayed, scene[0], scene[1], count)
        same_as_ref(eager, scene[0], scene[1], count)
        assert flag == ref["err"] == int(buf.error_flag.item())
    assert flag == _lib.BOX_ERR_RANGE                                 # (the last scene names 17 segments, 9 were asked for)
    with pytest.raises(ValueError):
        buf.check()
    with pytest.raises(ValueError):
        boxes.segment_boxes(pts_s, inv_s, segs, row_begin=begin, row_count=rows, max_rows=cap, buffers=boxes.buffers(cap, 1, cap, 32, dev))
    with pytest.raises(_lib.Pn2Error):
        boxes.segment_boxes(pts_s.cpu(), inv_s, segs)


def rotate_about(p, a, A=64):
    th = a * (math.pi / 2) / A
    Rm = np.array([[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]])
    return p @ Rm.T


def test_ground_removal_clustering_and_boxes_end_to_end(dev):
    """The ground lattice with two boxes of test_plane_gpu.py's clustering case, the boxes (12 x 6 x 6 lattices of 1/8 m) turned by the
    table angles 9 and 40: ``ground_labels`` -> ``euclidean_cluster`` -> ``instance_boxes`` gives two boxes with those angles."""
    g = np.mgrid[0:48, 0:48].reshape(2, -1).T / 8
    ground = np.concatenate([g, np.zeros((len(g), 1))], 1)
    box = np.mgrid[0:12, 0:6, 2:8].reshape(3, -1).T / 8
    rng = np.random.default_rng(7)
    pts = np.concatenate([ground, rotate_about(box, 9) + [1.0, 1.0, 0.0], rotate_about(box, 40) + [4.0, 2.5, 0.0]]).astype(np.float32)
    order = rng.permutation(len(pts))
    pts, is_ground = pts[order], (order < len(ground))
    d = torch.from_numpy(pts).to(dev)
    labels = plane.ground_labels(d, threshold=0.05, max_angle=15.0)
    assert np.array_equal(labels.cpu().numpy(), np.where(is_ground, -1, 0))
    comps, _, grid = voxel.euclidean_cluster(d, labels, voxel_size=0.25)
    assert int(comps.count[0]) == 2
    grid.check()
    b = boxes.instance_boxes(d, comps)
    got = as_numpy(b, 2)
    rc = comps.row_component.cpu().numpy()
    ref = same_as_ref(got, pts, rc, 2)
    left = 0 if ref["center"][0, 0] < ref["center"][1, 0] else 1     # (ids follow the lowest row: either box may be 0)
    assert got["angle"][left] == 9 and got["angle"][1 - left] == 40 and got["n"].tolist() == [432, 432]
    assert np.allclose(ref["size"], [[11 / 8, 5 / 8, 5 / 8]] * 2, atol=1e-5)
    c = boxes.canonical(b)
    assert torch.equal(c.size[:2], b.size[:2]) and boxes.corners(b).shape == (len(pts), 8, 3)
    inside = boxes.contains(b, d, comps.row_component, margin=1e-4).cpu().numpy()
    assert np.array_equal(inside, ~is_ground)


class Stub(torch.nn.Module):
    """A tiny stand-in for the network: ``[1, 4, n]`` -> log-probabilities ``[1, n, 19]``, constant over blocks in x and y so that
    neighbouring rows share a class (test_cluster_gpu.py's)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(64, 19, generator=torch.Generator().manual_seed(0)))

    def forward(self, x):
        block = (torch.floor(x[:, 0, :] * 8).long() * 5 + torch.floor(x[:, 1, :] * 8).long()) % 64
        return torch.log_softmax(self.w[block], -1)


def test_label_scan_with_instance_boxes(dev, monkeypatch):
    g9, g = golden("g9_kitti.npz"), golden("g18_kitti_view.npz")
    lmap = {int(k): int(v) for k, v in zip(g9["map_keys"], g9["map_values"])}
    raw, words = np.ascontiguousarray(g9["bin"]), np.ascontiguousarray(g9["label"])
    seg = V.FrameSegmenter(Stub().to(dev), V.Calibration(g["R"], g["T"], g["P"]), g["colors"], npoints=4096)
    sf = kitti.ScanFilter(lmap, "all", device=dev)
    raw_d, words_d = torch.from_numpy(raw).to(dev), torch.from_numpy(words.view(np.int32)).to(dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(5)
    plain = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=gen(), instances=V.InstanceSpec(0.5, range(8), min_points=3))
    keys, ids = set(plain), plain["kept_instances"].clone()
    assert "instance_boxes" not in keys                              # the default returns exactly the keys it returned before
    spec = V.InstanceSpec(0.5, range(8), min_points=3, boxes=True, box_angles=90, box_d0=0.1)
    out = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=gen(), instances=spec)
    torch.cuda.synchronize()
    assert set(out) == keys | {"instance_boxes"} and torch.equal(out["kept_instances"], ids)
    count, S = int(out["count"].item()), int(out["instance_count"].item())
    assert S > 5 and int(seg._raw_state["instances"]["grid"].error_flag.item()) == 0
    kept = SR.scan_filter(raw, words, SR.make_lut(lmap))
    got = as_numpy(out["instance_boxes"], S)
    same_as_ref(got, kept["points"], out["kept_instances"][:count].cpu().numpy(), S, A=90, d0=0.1)
    # the direct call on the same rows: the same Boxes
    pts = seg._raw_state["out"].points
    direct = boxes.segment_boxes(pts, out["kept_instances"], out["instance_count"], angles=90, d0=0.1, row_begin=seg._raw_state["begin"],
                                 row_count=out["count"], max_rows=int(pts.shape[0]))
    mine = as_numpy(direct, S)
    for name in NAMES:
        assert np.array_equal(mine[name], got[name]), name

    def forbidden(*args, **kwargs):
        raise AssertionError("label_scan read something back")
    with monkeypatch.context() as mp:
        for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "nonzero"):
            mp.setattr(torch.Tensor, name, forbidden)
        mp.setattr(torch.cuda, "synchronize", forbidden)
        again = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=gen(), instances=spec)
    torch.cuda.synchronize()
    for name in NAMES:
        assert np.array_equal(as_numpy(again["instance_boxes"], S)[name], got[name]), name
