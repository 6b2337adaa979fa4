"""GPU: the segment reductions (``pn2_segment_mean`` / ``pn2_segment_mean_bwd`` / ``pn2_segment_mode``, csrc/voxel_reduce.hip) and what
is built on them (``voxel.VoxelGrid(reduce="mean", label_reduce="mode")``, ``segment_mean`` / ``segment_mode`` / ``pool_mean``,
``frame_raw`` / ``load_scans`` with such a grid) against the numpy statement of their rules (tests/voxel_reduce_ref.py): RAW BITS
throughout.  Every ABI call runs with poisoned outputs and a 0xEE-filled workspace; every byte outside the written ranges must come
back untouched."""
import os

import numpy as np
import pytest
import torch

import scan_filter_ref as SR
import voxel_reduce_ref as R
import voxel_ref as VR
from conftest import golden
from pointnet12_amd import _lib, kitti, voxel
from pointnet12_amd import kitti_view as V

pytestmark = pytest.mark.gpu

POISON_F, POISON_I = 0x5A5A5A5A, -777
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 5000]
F32_MAX = np.finfo(np.float32).max


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def setup(dev, seg, begins, counts, out_counts, out_begins):
    t64 = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int64, device=dev)
    seg_d = torch.from_numpy(np.ascontiguousarray(seg, np.int32)).to(dev)
    return seg_d, t64(begins), t64(counts), t64(out_begins), t64(out_counts), torch.zeros(1, dtype=torch.int32, device=dev)


def workspace(dev, B, max_rows, C):
    nbytes = _lib.load().pn2_segment_reduce_workspace_bytes(B, max_rows, C)
    assert nbytes > 0
    return torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)


def written_rows(out_rows, out_begins, out_counts, max_rows):
    written = np.zeros(out_rows, bool)
    for ob, oc in zip(out_begins, out_counts):
        m = max(0, min(int(oc), max_rows))
        assert ob + m <= out_rows and not written[ob:ob + m].any()
        written[ob:ob + m] = True
    return written


def run_mean(dev, values, C, seg, begins, counts, max_rows, out_counts, out_begins=None, out_rows=None, n_points=None, in_offset=0,
             out_offset=0, ld_out=None):
    """One ``pn2_segment_mean`` call on host arrays: ``(out uint32 [out_rows, ld_out], n_out int32 [out_rows], err)``."""
    lib = _lib.load()
    values = np.ascontiguousarray(values, np.float32)
    rows, ld = values.shape
    B = len(begins)
    out_begins = list(begins) if out_begins is None else list(out_begins)
    out_rows = rows if out_rows is None else out_rows
    ld_out = ld if ld_out is None else ld_out
    flat = torch.zeros(rows * ld + in_offset, dtype=torch.float32, device=dev)
    flat[in_offset:].copy_(torch.from_numpy(values.reshape(-1)))
    seg_d, begin_d, count_d, ob_d, oc_d, err = setup(dev, seg, begins, counts, out_counts, out_begins)
    n_d = None if n_points is None else torch.from_numpy(np.ascontiguousarray(n_points, np.int32)).to(dev)
    out = torch.full((out_rows * ld_out + out_offset,), POISON_F, dtype=torch.int32, device=dev)
    n_out = torch.full((out_rows,), POISON_I, dtype=torch.int32, device=dev)
    ws = workspace(dev, B, max_rows, C)
    p = _lib.ptr
    rc = lib.pn2_segment_mean(flat.data_ptr() + 4 * in_offset, ld, C, p(seg_d), p(begin_d), p(count_d), B, max_rows, p(ob_d), p(oc_d), p(n_d),
                              out.data_ptr() + 4 * out_offset, ld_out, p(n_out), p(err), p(ws), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out_h = out.cpu().numpy().view(np.uint32)
    assert (out_h[:out_offset] == POISON_F).all()
    out_h = out_h[out_offset:].reshape(out_rows, ld_out)
    n_h = n_out.cpu().numpy()
    written = written_rows(out_rows, out_begins, out_counts, max_rows)
    assert (out_h[~written] == POISON_F).all() and (out_h[:, C:] == POISON_F).all(), "the mean wrote outside its rows or columns"
    assert (n_h[~written] == POISON_I).all()
    return out_h, n_h, int(err.item())


def check_mean(dev, values, C, seg, begins, counts, max_rows, out_counts, **kw):
    """``run_mean`` against the restatement, cloud by cloud: bits, the counted rows, the error word."""
    out_begins = kw.get("out_begins") or list(begins)
    n_points = kw.get("n_points")
    out, n, err = run_mean(dev, values, C, seg, begins, counts, max_rows, out_counts, **kw)
    values, seg = np.ascontiguousarray(values, np.float32), np.asarray(seg)
    expect_err = 0
    for b in range(len(begins)):
        c, m = max(0, min(int(counts[b]), max_rows)), max(0, min(int(out_counts[b]), max_rows))
        lo, ob = begins[b], out_begins[b]
        ref = R.segment_mean(values[lo:lo + c, :C], seg[lo:lo + c], m, None if n_points is None else n_points[ob:ob + m])
        expect_err |= ref["err"]
        assert np.array_equal(out[ob:ob + m, :C], u32(ref["mean"])), "cloud %d" % b
        assert np.array_equal(n[ob:ob + m], ref["n"])
    assert err == expect_err
    return out, n, err


def run_mode(dev, labels, seg, begins, counts, max_rows, out_counts, out_begins=None, out_rows=None, fill=-1, want=("labels", "votes")):
    lib = _lib.load()
    rows, B = len(labels), len(begins)
    out_begins = list(begins) if out_begins is None else list(out_begins)
    out_rows = rows if out_rows is None else out_rows
    lab_d = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
    seg_d, begin_d, count_d, ob_d, oc_d, err = setup(dev, seg, begins, counts, out_counts, out_begins)
    out, votes = (torch.full((out_rows,), POISON_I, dtype=torch.int32, device=dev) for _ in range(2))
    ws = workspace(dev, B, max_rows, 1)
    p = _lib.ptr
    rc = lib.pn2_segment_mode(p(lab_d), p(seg_d), p(begin_d), p(count_d), B, max_rows, p(ob_d), p(oc_d), fill,
                              p(out) if "labels" in want else None, p(votes) if "votes" in want else None, p(err), p(ws), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out_h, votes_h = out.cpu().numpy(), votes.cpu().numpy()
    written = written_rows(out_rows, out_begins, out_counts, max_rows)
    for name, arr in (("labels", out_h), ("votes", votes_h)):
        assert (arr[~written] == POISON_I).all() if name in want else (arr == POISON_I).all(), "%s written outside its rows" % name
    return out_h, votes_h, int(err.item())


def check_mode(dev, labels, seg, begins, counts, max_rows, out_counts, fill=-1, **kw):
    out_begins = kw.get("out_begins") or list(begins)
    want = kw.get("want", ("labels", "votes"))
    out, votes, err = run_mode(dev, labels, seg, begins, counts, max_rows, out_counts, fill=fill, **kw)
    labels, seg = np.asarray(labels), np.asarray(seg)
    expect_err = 0
    for b in range(len(begins)):
        c, m = max(0, min(int(counts[b]), max_rows)), max(0, min(int(out_counts[b]), max_rows))
        lo, ob = begins[b], out_begins[b]
        w, v, e = R.segment_mode(labels[lo:lo + c], seg[lo:lo + c], m, fill)
        expect_err |= e
        assert "labels" not in want or np.array_equal(out[ob:ob + m], w), "cloud %d" % b
        assert "votes" not in want or np.array_equal(votes[ob:ob + m], v), "cloud %d" % b
    assert err == expect_err
    return out, votes, err


def check_bwd(dev, grad_out, C, seg, begins, counts, max_rows, out_counts, n_points, out_begins=None, rows=None, ld_in=None):
    """One ``pn2_segment_mean_bwd`` call against ``float32(g) / float32(n)``: bits; rows outside the clouds and columns beyond C keep
    the poison."""
    lib = _lib.load()
    grad_out = np.ascontiguousarray(grad_out, np.float32)
    out_rows, ld_out = grad_out.shape
    rows = len(seg) if rows is None else rows
    ld_in = C if ld_in is None else ld_in
    out_begins = list(begins) if out_begins is None else list(out_begins)
    g_d = torch.from_numpy(grad_out).to(dev)
    n_d = torch.from_numpy(np.ascontiguousarray(n_points, np.int32)).to(dev)
    seg_d, begin_d, count_d, ob_d, oc_d, err = setup(dev, seg, begins, counts, out_counts, out_begins)
    gin = torch.full((rows, ld_in), POISON_F, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = lib.pn2_segment_mean_bwd(p(g_d), ld_out, C, p(seg_d), p(begin_d), p(count_d), len(begins), max_rows, p(ob_d), p(oc_d), p(n_d), p(gin),
                                  ld_in, p(err), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = gin.cpu().numpy().view(np.uint32)
    inside, expect_err, seg = np.zeros(rows, bool), 0, np.asarray(seg)
    for b in range(len(begins)):
        c, m = max(0, min(int(counts[b]), max_rows)), max(0, min(int(out_counts[b]), max_rows))
        lo, ob = begins[b], out_begins[b]
        inside[lo:lo + c] = True
        ref, e = R.segment_mean_bwd(grad_out[ob:ob + m, :C] if m else np.zeros((1, C), np.float32), seg[lo:lo + c], m, n_points[ob:ob + max(m, 1)])
        expect_err |= e
        assert np.array_equal(got[lo:lo + c, :C], u32(ref)), "cloud %d" % b
    assert (got[~inside] == POISON_F).all() and (got[:, C:] == POISON_F).all() and int(err.item()) == expect_err
    return got


class options:
    """``with options(PN2_NAME=value, ...):`` library options for the block, restored afterwards."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.old = {k: _lib.options()[k] for k in self.values}
        for k, v in self.values.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _lib.set_option(k, v)
        return False


def mixed_values(rng, M, ld):
    """Finite float32 rows whose columns spread over a few decades, signs mixed."""
    return (rng.normal(size=(M, ld)) * 10.0 ** rng.uniform(-3, 3, size=(M, ld))).astype(np.float32)


def memberships(rng, M):
    """{name: (seg, count)}: the four membership patterns."""
    lengths = rng.integers(1, 150, size=M)                           # runs of equal segment that cross wave and tile borders;
    ids = rng.integers(0, M // 40 + 2, size=M)                       # a segment comes back in later runs
    runs = np.repeat(ids, lengths)[:M].astype(np.int32)
    return {"one": (np.zeros(M, np.int32), 1), "own": (rng.permutation(M).astype(np.int32), M), "runs": (runs, M // 40 + 2),
            "mod7": ((np.arange(M) % 7).astype(np.int32), 7)}


@pytest.mark.parametrize("pattern", ["one", "own", "runs", "mod7"])
@pytest.mark.parametrize("M", SIZES)
def test_sizes_and_membership_patterns(dev, M, pattern):
    rng = np.random.default_rng(M)
    values = mixed_values(rng, M, 4)
    labels = rng.integers(-1, 5, M).astype(np.int32)
    seg, count = memberships(rng, M)[pattern]
    bound, out_rows = max(M, count), max(M, count) + 3               # (i % 7 names seven segments even for one row: six stay empty)
    out, n, err = check_mean(dev, values, 4, seg, [0], [M], bound, [count], out_rows=out_rows)
    assert err == 0 and n[:count].sum() == M
    check_mode(dev, labels, seg, [0], [M], bound, [count], out_rows=out_rows)
    grad = mixed_values(rng, count, 4)
    check_bwd(dev, grad, 4, seg, [0], [M], bound, [count], n[:count])
    # a caller's n_points is used as it is; a bound above the count changes nothing
    given = rng.integers(0, 9, count).astype(np.int32)
    check_mean(dev, values, 4, seg, [0], [M], bound + 37, [count], n_points=given, out_rows=out_rows)
    check_bwd(dev, grad, 4, seg, [0], [M], bound + 37, [count], given)


@pytest.mark.parametrize("ld,C,in_offset,out_offset", [(3, 3, 0, 0), (3, 2, 1, 0), (4, 4, 1, 3), (4, 3, 0, 1), (6, 6, 1, 1), (6, 1, 0, 0),
                                                       (9, 9, 3, 2), (9, 5, 0, 0), (16, 16, 1, 0), (16, 11, 0, 3)])
def test_row_widths_columns_and_misaligned_offsets(dev, ld, C, in_offset, out_offset):
    rng = np.random.default_rng(ld * 100 + C)
    M = 1025
    values = mixed_values(rng, M, ld)
    seg, count = memberships(rng, M)["runs"]
    seg[rng.integers(0, M, 30)] = -1                                 # rows that take no part
    out, n, err = check_mean(dev, values, C, seg, [0], [M], M, [count], in_offset=in_offset, out_offset=out_offset)
    assert err == 0 and n[:count].sum() == (seg >= 0).sum()
    check_mean(dev, values, C, seg, [0], [M], M, [count], in_offset=in_offset, out_offset=out_offset, ld_out=C)   # another output pitch
    grad = mixed_values(rng, count, ld)
    check_bwd(dev, grad, C, seg, [0], [M], M, [count], n[:count], ld_in=ld)
    check_bwd(dev, grad, C, seg, [0], [M], M, [count], n[:count])


def test_special_values_and_a_non_finite_column(dev):
    rng = np.random.default_rng(7)
    M, count = 700, 9
    seg = rng.integers(0, count, M).astype(np.int32)
    tiny = np.float32(2.0 ** -149)
    v = np.zeros((M, 8), np.float32)
    v[:, 0] = np.where(rng.integers(0, 2, M) == 1, 0.0, -0.0)                                        # +-0 only: +0.0
    v[:, 1] = (rng.integers(-(1 << 23) + 1, 1 << 23, M) * 2.0 ** -149).astype(np.float32)            # subnormals
    v[:, 2] = np.where(rng.integers(0, 4, M) == 0, -F32_MAX, F32_MAX)                                # a float32 sum would overflow
    v[:, 3] = (rng.normal(size=M) * 10.0 ** rng.uniform(-38, 38, M)).astype(np.float32)              # spreads far above 2^34
    v[:, 4] = np.where(np.arange(M) % 50 == 0, np.float32(2.0 ** 40), rng.normal(size=M).astype(np.float32) * tiny * 1000)
    v[:, 5] = np.where(np.arange(M) % 2 == 0, np.float32(1.75), np.float32(-1.75))                   # x, -x
    v[:, 6] = (rng.uniform(-4, 4, M) * 2.0 ** -126).astype(np.float32)                               # around the smallest normal
    v[:, 7] = rng.normal(size=M).astype(np.float32)
    v[seg == 2, 5] = np.float32(3.5) * np.where(np.arange((seg == 2).sum()) % 2 == 0, 1, -1)
    out, n, err = check_mean(dev, v, 8, seg, [0], [M], M, [count])
    assert err == 0 and (out[:count, 0] == 0).all() and np.isfinite(out[:count].view(np.float32)).all()
    # NaN, +inf and -inf in ONE column of ONE segment each: that column is the quiet NaN, its neighbours are untouched
    for bad_value in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[np.flatnonzero(seg == 4)[3], 3] = bad_value
        got, _, err = check_mean(dev, w, 8, seg, [0], [M], M, [count])
        assert err == _lib.SEGMENT_ERR_NONFINITE and got[4, 3] == R.QUIET_NAN
        expect = out[:count, :8].copy()
        expect[4, 3] = R.QUIET_NAN
        assert np.array_equal(got[:count, :8], expect)
    w = v.copy()
    rows4 = np.flatnonzero(seg == 4)
    w[rows4[0], 7], w[rows4[1], 7] = np.inf, -np.inf
    got, _, err = check_mean(dev, w, 8, seg, [0], [M], M, [count])
    assert err == _lib.SEGMENT_ERR_NONFINITE and got[4, 7] == R.QUIET_NAN and np.array_equal(got[:count, :7], out[:count, :7])


def test_three_clouds_with_identical_values_do_not_mix(dev):
    rng = np.random.default_rng(5)
    counts, begins = [0, 1, 700], [3, 3, 10]
    rows = 10 + 700 + 9
    base = mixed_values(rng, 700, 4)
    base_seg = rng.integers(0, 60, 700).astype(np.int32)
    base_lab = rng.integers(0, 4, 700).astype(np.int32)
    values, seg, labels = mixed_values(rng, rows, 4), rng.integers(0, 60, rows).astype(np.int32), rng.integers(0, 4, rows).astype(np.int32)
    for b, c in zip(begins, counts):
        values[b:b + c], seg[b:b + c], labels[b:b + c] = base[:c], base_seg[:c], base_lab[:c]       # the SAME rows in every cloud
    out_counts = [0, int(base_seg[0]) + 1, 60]
    out_begins, out_rows = [5, 100, 7], 100 + 60 + 11
    out, n, err = check_mean(dev, values, 4, seg, begins, counts, 700, out_counts, out_begins=out_begins, out_rows=out_rows)
    assert err == 0 and n[100 + base_seg[0]] == 1 and np.array_equal(out[100 + base_seg[0], :4], u32(base[0]))   # a one-row mean is the row
    lab, votes, err = check_mode(dev, labels, seg, begins, counts, 700, out_counts, out_begins=out_begins, out_rows=out_rows)
    assert err == 0 and lab[100 + base_seg[0]] == base_lab[0] and votes[100 + base_seg[0]] == 1
    check_bwd(dev, mixed_values(rng, out_rows, 4), 4, seg, begins, counts, 700, out_counts, np.maximum(n, 0), out_begins=out_begins)
    # a row_count above max_rows is clamped: the rows beyond take no part
    check_mean(dev, values, 4, seg, begins, counts, 512, out_counts, out_begins=out_begins, out_rows=out_rows)
    check_mode(dev, labels, seg, begins, counts, 512, out_counts, out_begins=out_begins, out_rows=out_rows)


def test_a_segment_beyond_the_count_sets_the_bit_and_writes_nothing_outside(dev):
    """Canary rows follow each cloud's output range (``run_mean`` / ``run_mode`` poison them and look)."""
    rng = np.random.default_rng(8)
    counts, begins = [300, 200], [0, 300]
    values, labels = mixed_values(rng, 500, 4), rng.integers(0, 9, 500).astype(np.int32)
    seg = rng.integers(0, 20, 500).astype(np.int32)
    out_counts, out_begins, out_rows = [20, 20], [0, 24], 48         # four canary rows behind each range
    _, _, err = check_mean(dev, values, 4, seg, begins, counts, 300, out_counts, out_begins=out_begins, out_rows=out_rows)
    assert err == 0
    for value in (20, 21, 24, 299, 300, 10 ** 6, 2 ** 31 - 1):       # at the count, inside the NEXT cloud's range, at max_rows, far beyond
        s = seg.copy()
        s[[7, 150, 299]] = value
        _, _, err = check_mean(dev, values, 4, s, begins, counts, 300, out_counts, out_begins=out_begins, out_rows=out_rows)
        assert err == _lib.SEGMENT_ERR_RANGE
        _, _, err = check_mode(dev, labels, s, begins, counts, 300, out_counts, out_begins=out_begins, out_rows=out_rows)
        assert err == _lib.SEGMENT_ERR_RANGE
        check_bwd(dev, mixed_values(rng, out_rows, 4), 4, s, begins, counts, 300, out_counts, np.ones(out_rows, np.int32), out_begins=out_begins)
    # an out_count above max_rows is clamped to it
    check_mean(dev, values, 4, seg, begins, counts, 300, [10 ** 9, 20], out_begins=[0, 300], out_rows=320 + 300)


def test_mode_cases(dev):
    # ties go to the LOWEST label, negative labels do not vote, a segment of negatives gets `fill`, an empty one too
    labels = [5, 5, 2, 2, 9,   -1, -7, -1,   2 ** 31 - 1, 2 ** 31 - 1, 0,   3, -1, -1, -1,   1, 0]
    seg = [0, 0, 0, 0, 0,      1, 1, 1,      2, 2, 2,                       4, 4, 4, 4,      5, 5]
    out, votes, err = check_mode(dev, labels, seg, [0], [len(seg)], 32, [6], fill=-9, out_rows=8)
    assert err == 0 and out[:6].tolist() == [2, -9, 2 ** 31 - 1, -9, 3, 0] and votes[:6].tolist() == [2, 0, 2, 0, 1, 1]
    # every row of a segment with a label of its own: the lowest wins with one vote; beside it a segment with one heavy label
    rng = np.random.default_rng(3)
    M = 3000
    labels = rng.permutation(M).astype(np.int32) + 17
    seg = np.zeros(M, np.int32)
    seg[2000:] = 1
    labels[2000:] = rng.integers(0, 3, 1000)
    out, votes, err = check_mode(dev, labels, seg, [0], [M], M, [2])
    assert out[0] == labels[:2000].min() and votes[0] == 1 and votes[1] == np.bincount(labels[2000:]).max()
    # each optional output alone
    check_mode(dev, labels, seg, [0], [M], M, [2], want=("labels",))
    check_mode(dev, labels, seg, [0], [M], M, [2], want=("votes",))
    # many classes, random membership: the table at work
    seg = rng.integers(-1, 400, M).astype(np.int32)
    labels = rng.integers(-3, 2000, M).astype(np.int32)
    check_mode(dev, labels, seg, [0], [M], M, [400])
    out = voxel.segment_mode(torch.from_numpy(labels).to(dev), torch.from_numpy(seg).to(dev), 400, fill=-4, return_votes=True)
    w, v, _ = R.segment_mode(labels, seg, 400, -4)
    assert np.array_equal(out[0][:400].cpu().numpy(), w) and np.array_equal(out[1][:400].cpu().numpy(), v) and (out[0][400:] == -4).all()


def reduced_ref(cloud, labels, size):
    """The grid with mean and mode on one cloud, in numpy: voxel_ref's dict plus ``mean`` (bits), ``mode`` and ``votes``."""
    ref = VR.voxel_grid(cloud, 0.0, size, labels)
    m = R.segment_mean(cloud, ref["inverse"], ref["count"])
    assert np.array_equal(m["n"], ref["n_points"])
    ref["mean"], ref["mean_err"] = u32(m["mean"]), m["err"]
    if labels is not None:
        ref["mode"], ref["votes"], _ = R.segment_mode(labels, ref["inverse"], ref["count"])
    return ref


def downsample_np(vg, dev, cloud, labels, bufs=None):
    """``vg.downsample`` of one host cloud -> numpy dict (the first ``count`` rows of every output)."""
    lab = None if labels is None else torch.from_numpy(labels).to(dev)
    p, l, i, c, inv, pop = vg.downsample(torch.from_numpy(cloud).to(dev), lab, out=bufs)
    m = int(c.item())
    return {"points": u32(p[:m].cpu().numpy()), "labels": None if l is None else l[:m].cpu().numpy(), "index": i[:m].cpu().numpy(),
            "count": m, "inverse": inv.cpu().numpy(), "n_points": pop[:m].cpu().numpy()}


def test_same_cloud_twice_and_row_permuted(dev):
    rng = np.random.default_rng(9)
    M = 20000
    cloud = rng.normal(size=(M, 4)).astype(np.float32)
    cloud[:, :3] = rng.uniform(-1.6, 2.4, size=(M, 3)).astype(np.float32)         # about four rows per 0.25 cell
    labels = rng.integers(0, 6, M).astype(np.int32)
    vg = voxel.VoxelGrid(0.25, device=dev, reduce="mean", label_reduce="mode")
    bufs = vg.buffers(M)
    runs = []
    for _ in range(2):
        got = downsample_np(vg, dev, cloud, labels, bufs)
        got["votes"] = bufs.votes[:got["count"]].cpu().numpy()
        runs.append(got)
        bufs.points.fill_(7.0)
    for name in ("points", "labels", "votes", "index", "inverse", "n_points"):
        assert np.array_equal(runs[0][name], runs[1][name]), name
    ref = reduced_ref(cloud, labels, 0.25)
    assert np.array_equal(runs[0]["points"], ref["mean"]) and np.array_equal(runs[0]["labels"], ref["mode"])
    assert np.array_equal(runs[0]["votes"], ref["votes"]) and (ref["n_points"] > 1).sum() > 1000
    perm = rng.permutation(M)
    back = downsample_np(vg, dev, cloud[perm], labels[perm], bufs)
    back["votes"] = bufs.votes[:back["count"]].cpu().numpy()
    assert back["count"] == runs[0]["count"] and int(vg.error_flag.item()) == 0
    # per cell KEY (of each voxel's representative row): the same means, winners and votes, byte for byte
    key_a = VR.keys(cloud[runs[0]["index"]], 0.0, 0.25)[0]
    key_b = VR.keys(cloud[perm][back["index"]], 0.0, 0.25)[0]
    a, b = np.argsort(key_a), np.argsort(key_b)
    assert np.array_equal(key_a[a], key_b[b])
    for name in ("points", "labels", "votes", "n_points"):
        assert np.array_equal(runs[0][name][a], back[name][b]), name
    # with and without the wave's run combining, with either lane mapping: the same bytes
    for combine, lanes in ((0, 1), (1, 0), (0, 0)):
        with options(PN2_SEGRED_COMBINE=combine, PN2_SEGRED_LANES=lanes):
            other = downsample_np(vg, dev, cloud, labels, bufs)
            other["votes"] = bufs.votes[:other["count"]].cpu().numpy()
        for name in ("points", "labels", "votes", "n_points"):
            assert np.array_equal(runs[0][name], other[name]), (name, combine, lanes)


@pytest.mark.parametrize("combine,lanes", [(0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("C", [1, 3, 4, 16])
def test_every_form_of_the_row_passes_against_the_restatement(dev, C, combine, lanes):
    """Options SEGRED_COMBINE / SEGRED_LANES pick among four forms of the mean's two row passes (and two of the mode's insert);
    the defaults run everywhere else in this file."""
    rng = np.random.default_rng(C)
    for M in (65, 1025):
        values = mixed_values(rng, M, C)
        labels = rng.integers(-1, 4, M).astype(np.int32)
        for pattern, (seg, count) in memberships(rng, M).items():
            with options(PN2_SEGRED_COMBINE=combine, PN2_SEGRED_LANES=lanes):
                check_mean(dev, values, C, seg, [0], [M], max(M, count), [count], out_rows=max(M, count))
                check_mode(dev, labels, seg, [0], [M], max(M, count), [count], out_rows=max(M, count))


def test_backward_and_pool_mean_through_autograd(dev):
    rng = np.random.default_rng(12)
    M, C, count = 300, 8, 37
    feats = mixed_values(rng, M, C)
    seg = rng.integers(-1, count, M).astype(np.int32)
    seg[seg == 5] = 6                                                # segment 5: empty
    weight = mixed_values(rng, M, C)
    x = torch.from_numpy(feats).to(dev).requires_grad_(True)
    inv = torch.from_numpy(seg).to(dev)
    pooled = voxel.pool_mean(x, inv, count)
    assert pooled.shape == (M, C) and pooled.requires_grad
    ref = R.segment_mean(feats, seg, count)
    assert np.array_equal(u32(pooled.detach()[:count].cpu().numpy()), u32(ref["mean"])) and not pooled.detach()[count:].any()
    (pooled * torch.from_numpy(weight).to(dev)).sum().backward()
    expect, _ = R.segment_mean_bwd(weight[:count], seg, count, ref["n"])
    assert np.array_equal(u32(x.grad.cpu().numpy()), u32(expect))
    assert not x.grad[torch.from_numpy(seg < 0).to(dev)].any()       # zeros for rows outside any segment
    # the stand-alone mean with the grid's own n_points and a device-side count
    count_d = torch.tensor([count], dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    got = voxel.segment_mean(x.detach(), inv, count_d, n_points=torch.from_numpy(ref["n"]).to(dev), error_flag=err)
    assert np.array_equal(u32(got[:count].cpu().numpy()), u32(ref["mean"])) and int(err.item()) == 0
    # batched: two clouds back to back, outputs elsewhere
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    both = voxel.pool_mean(x.detach().clone().requires_grad_(True), inv, t64([count, count]), row_begin=t64([0, 150]), row_count=t64([150, 150]),
                           max_rows=150, out_begin=t64([40, 0]), out_rows=80)
    for b, (lo, ob) in enumerate(((0, 40), (150, 0))):
        r = R.segment_mean(feats[lo:lo + 150], seg[lo:lo + 150], count)
        assert np.array_equal(u32(both.detach()[ob:ob + count].cpu().numpy()), u32(r["mean"])), b


def test_capture_and_replay_with_other_rows_and_count(dev):
    rng = np.random.default_rng(21)
    cap = 3 * 1024 + 17

    def make(M):
        c = rng.normal(size=(M, 4)).astype(np.float32)
        c[:, :3] = rng.uniform(-0.6, 0.9, size=(M, 3)).astype(np.float32)
        return c, rng.integers(0, 19, M).astype(np.int32)

    (cloud_a, lab_a), (cloud_b, lab_b) = make(cap), make(2 * 1024 + 3)
    vg = voxel.VoxelGrid(0.1, device=dev, reduce="mean", label_reduce="mode")
    bufs = vg.buffers(cap)
    assert bufs.reduce_workspace is not None and voxel.VoxelGrid(0.1, device=dev).buffers(cap).reduce_workspace is None
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
        return {"points": u32(bufs.points[:m].cpu().numpy()), "labels": bufs.labels[:m].cpu().numpy(), "votes": bufs.votes[:m].cpu().numpy(),
                "index": bufs.index[:m].cpu().numpy(), "n_points": bufs.n_points[:m].cpu().numpy(),
                "inverse": bufs.inverse[:rows].cpu().numpy(), "count": m}

    def same(ref, got):
        assert got["count"] == ref["count"] and np.array_equal(got["points"], ref["mean"]) and np.array_equal(got["labels"], ref["mode"])
        assert np.array_equal(got["votes"], ref["votes"])
        for name in ("index", "inverse", "n_points"):
            assert np.array_equal(got[name], ref[name]), name

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
    for cloud, lab in ((cloud_b, lab_b), (cloud_a, lab_a), (cloud_b[:1023], lab_b[:1023])):
        load(cloud, lab)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before               # nothing allocated by a replay
        replayed = snapshot()
        bufs.count.zero_()
        bufs.points.fill_(3.0)
        bufs.labels.fill_(POISON_I)
        step()
        eager = snapshot()
        ref = reduced_ref(cloud, lab, 0.1)
        same(ref, replayed)
        same(ref, eager)
        assert int(vg.error_flag.item()) == 0
    # a buffer made by a grid that does not reduce is refused, and check() names the reductions' bit
    with pytest.raises(ValueError):
        vg.downsample(pts_s, lab_s, begin, count, cap, out=voxel.VoxelGrid(0.1, device=dev).buffers(cap))
    pts_s[5, 3] = float("nan")                                       # remission: no coordinate, the row stays in its voxel
    step()
    assert int(vg.error_flag.item()) == _lib.SEGMENT_ERR_NONFINITE
    with pytest.raises(ValueError):
        vg.check()


@pytest.mark.parametrize("size,count", [(0.1, 4800), (0.05, 5133), (0.2, 4116), (0.5, 3105)])
def test_recorded_scan(dev, size, count):
    g9 = golden("g9_kitti.npz")
    raw = np.ascontiguousarray(g9["bin"])
    labels = (np.ascontiguousarray(g9["label"]).view(np.uint32) & 0xFFFF).astype(np.int32).reshape(-1)
    assert len(labels) == len(raw) and len(np.unique(labels)) > 3
    ref = reduced_ref(raw, labels, size)
    first = downsample_np(voxel.VoxelGrid(size, device=dev), dev, raw, labels)
    vg = voxel.VoxelGrid(size, device=dev, reduce="mean", label_reduce="mode")
    got = downsample_np(vg, dev, raw, labels)
    assert got["count"] == count == ref["count"] and int(vg.error_flag.item()) == 0
    assert np.array_equal(got["points"], ref["mean"]) and np.array_equal(got["labels"], ref["mode"])
    for name in ("index", "inverse", "n_points"):                    # byte for byte what reduce="first" gives
        assert np.array_equal(got[name], first[name]) and np.array_equal(got[name], ref[name]), name
    assert np.array_equal(first["points"], u32(ref["points"])) and np.array_equal(first["labels"], ref["labels"])
    # each reduction alone; a mean without labels
    only_mean = downsample_np(voxel.VoxelGrid(size, device=dev, reduce="mean"), dev, raw, labels)
    assert np.array_equal(only_mean["points"], ref["mean"]) and np.array_equal(only_mean["labels"], ref["labels"])
    only_mode = downsample_np(voxel.VoxelGrid(size, device=dev, label_reduce="mode"), dev, raw, labels)
    assert np.array_equal(only_mode["points"], u32(ref["points"])) and np.array_equal(only_mode["labels"], ref["mode"])
    bare = downsample_np(vg, dev, raw, None)
    assert bare["labels"] is None and np.array_equal(bare["points"], ref["mean"])
    # the mean lies inside its cell: one rounding away at the most
    centre = ref["mean"].view(np.float32)[:, :3].astype(np.float64)
    cell = np.floor(raw[ref["index"], :3].astype(np.float64) / size)
    assert (centre >= cell * size - 1e-5).all() and (centre <= (cell + 1) * size + 1e-5).all()


class Stub(torch.nn.Module):
    """A tiny stand-in for the network: ``[1, 4, n]`` -> log-probabilities ``[1, n, 19]``."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(4, 19, generator=torch.Generator().manual_seed(0)))

    def forward(self, x):
        return torch.log_softmax(x.transpose(2, 1) @ self.w, -1)


def test_frame_raw_sees_the_means_of_the_kept_rows_voxels(dev):
    g9, g = golden("g9_kitti.npz"), golden("g18_kitti_view.npz")
    lmap = {int(k): int(v) for k, v in zip(g9["map_keys"], g9["map_values"])}
    raw, words = np.ascontiguousarray(g9["bin"]), np.ascontiguousarray(g9["label"])
    n = 4096
    seg = V.FrameSegmenter(Stub().to(dev), V.Calibration(g["R"], g["T"], g["P"]), g["colors"], npoints=n)
    sf = kitti.ScanFilter(lmap, "all", device=dev)
    kept = SR.scan_filter(raw, words, SR.make_lut(lmap))
    ref = reduced_ref(np.ascontiguousarray(kept["points"]), None, 0.2)
    count = ref["count"]
    assert 0 < count <= n < len(kept["points"])
    first = seg.frame_raw(raw, words, scan_filter=sf, rng="cover", voxel=voxel.VoxelGrid(0.2, device=dev))   # (its buffers have no workspace)
    first_rows = first["pts_3d"].clone()                             # (the result lives in the segmenter's static buffers)
    vg = voxel.VoxelGrid(0.2, device=dev, reduce="mean")
    out = seg.frame_raw(raw, words, scan_filter=sf, rng="cover", voxel=vg)
    assert int(seg.error_flag.item()) == 0 and int(sf.error_flag.item()) == 0 and int(vg.error_flag.item()) == 0
    assert int(out["voxel_count"].item()) == count
    drawn = np.arange(n) % count
    assert np.array_equal(u32(out["pts_3d"].cpu().numpy()), ref["mean"][drawn][:, :3])
    assert np.array_equal(u32(seg.raw_rows.cpu().numpy()), ref["mean"][drawn])
    assert np.array_equal(u32(first_rows.cpu().numpy()), u32(ref["points"])[drawn][:, :3]) and (ref["n_points"] > 1).sum() > 100
    assert not np.array_equal(u32(first_rows.cpu().numpy()), ref["mean"][drawn][:, :3])
    # voxel_index still names the representative, voxel_inverse is the grid's
    assert np.array_equal(out["voxel_index"][:count].cpu().numpy(), kept["index"][ref["index"]])
    assert np.array_equal(out["voxel_inverse"][:len(kept["points"])].cpu().numpy(), ref["inverse"])
    assert torch.equal(out["voxel_index"][:count], first["voxel_index"][:count])
    d = seg.label_scan(raw, words, scan_filter=sf, rng="cover", voxel=vg, max_dist=None)
    assert d["scan_labels"].shape == (len(raw),) and int(d["voxel_count"].item()) == count


def test_load_scans_device_ingest_with_a_reducing_grid(dev, tmp_path):
    g9 = golden("g9_kitti.npz")
    lmap = {int(k): int(v) for k, v in zip(g9["map_keys"], g9["map_values"])}
    raw, words = SR.decided_scan(31, 5000, classes=sorted(lmap))
    pairs, at = [], 0
    for k, m in enumerate((1031, 0, 3000)):
        fv, fl = os.path.join(tmp_path, "%06d.bin" % k), os.path.join(tmp_path, "%06d.label" % k)
        raw[at:at + m].tofile(fv)
        words[at:at + m].tofile(fl)
        pairs.append((fv, fl))
        at += m
    vg = voxel.VoxelGrid(8.0, device=dev, reduce="mean", label_reduce="mode")
    refs = []
    for fv, fl in pairs:
        p, l = kitti.read_scan(fv, fl, lmap, "all")
        refs.append(reduced_ref(np.ascontiguousarray(p, np.float32), np.ascontiguousarray(l, np.int32), 8.0) if len(p) else None)
    want_p = np.concatenate([r["mean"] for r in refs if r is not None], 0)
    want_l = np.concatenate([r["mode"] for r in refs if r is not None], 0)
    store = kitti.load_scans(pairs, lmap, "all", device=dev, ingest="device", voxel=vg)
    assert store.row_count.tolist() == [0 if r is None else r["count"] for r in refs]
    assert np.array_equal(u32(store.raw.cpu().numpy()), want_p) and np.array_equal(store.label.cpu().numpy(), want_l)
