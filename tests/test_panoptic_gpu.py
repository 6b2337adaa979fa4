"""GPU: ``pn2_panoptic_count`` (csrc/panoptic.hip) and what is built on it (``metrics.panoptic_counts`` / ``panoptic_scores`` /
``PanopticEvaluator``) against the numpy statement of the rule (tests/panoptic_ref.py) and against hand-worked literals: the table is
compared as EXACT int64, there is no tolerance anywhere.  Every ABI call adds into a table that already holds numbers, between
sentinel words; its workspace has exactly ``pn2_panoptic_workspace_bytes`` bytes, NaN-filled, with guard words behind; the rows
outside the clouds hold poison that would count if it were read."""
import numpy as np
import pytest
import torch

import panoptic_ref as R
from pointnet12_amd import _lib, kitti, metrics

pytestmark = pytest.mark.gpu

SENTINEL = -0x5A5A5A5A5A5A5A5B
GUARD = 0x6B
POISON_ID = 424242                                                   # an id no case uses, under a class that counts: one fat matched segment
GAP = 7                                                              # poison rows before, between and behind the clouds
CALL = ("include", "things", "min_points")


def layout(case):
    """The case's clouds moved apart: ``(four int32 arrays, begins, counts)`` with ``GAP`` poison rows around every cloud and the rows
    beyond the last count (room for a bound 128 above it) poisoned too."""
    begins = case.get("begins") or [0]
    counts = case.get("counts") or [len(case["gt_sem"])]
    inc = case.get("include")
    cls = case["C"] - 1 if inc is None else int(np.flatnonzero(np.asarray(inc))[-1])
    POISON = (cls, POISON_ID, cls, POISON_ID)
    cols = [[] for _ in range(4)]
    new_begins, at = [], 0
    for b, (lo, n) in enumerate(zip(begins, counts)):
        for k, name in enumerate(("pred_sem", "pred_inst", "gt_sem", "gt_inst")):
            cols[k] += [np.full(GAP, POISON[k], np.int64), np.asarray(case[name], np.int64)[lo:lo + n]]
        at += GAP
        new_begins.append(at)
        at += n
    arrays = [np.concatenate(c + [np.full(GAP + max(counts) + 128, POISON[k], np.int64)]).astype(np.int32) for k, c in enumerate(cols)]
    return arrays, new_begins, list(counts)


def mask(values, dev):
    return None if values is None else torch.from_numpy(np.asarray(values, np.int32)).to(dev)


def call(dev, arrays, begins, counts, C, include=None, things=None, min_points=30, max_rows=None, per_cloud=False, base=None, rows=None):
    """One ``pn2_panoptic_count`` call: ``(table as int64 array MINUS what it held, err)``; asserts sentinels and guards."""
    lib = _lib.load()
    B = len(begins)
    max_rows = max(counts + [0]) if max_rows is None else max_rows
    d = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev) for a in arrays]
    t64 = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int64, device=dev)
    begin_d, count_d = t64(begins), t64(counts)
    words = (B if per_cloud else 1) * C * 5
    held = np.arange(words, dtype=np.int64) * 3 + 11 if base is None else base
    table = torch.full((words + 8,), SENTINEL, dtype=torch.int64, device=dev)
    table[4:4 + words] = torch.from_numpy(held).to(dev)
    nbytes = lib.pn2_panoptic_workspace_bytes(B, max_rows)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes // 4 + 16,), float("nan"), dtype=torch.float32, device=dev)
    ws[nbytes // 4:] = torch.tensor([GUARD], dtype=torch.int32, device=dev).view(torch.float32)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    inc = mask(np.ones(C, np.int32) if include is None else include, dev)
    p = _lib.ptr
    rc = lib.pn2_panoptic_count(p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(begin_d), p(count_d), B, max_rows,
                                len(arrays[0]) if rows is None else rows, C, p(inc), p(mask(things, dev)), min_points,
                                table.data_ptr() + 32, 5 * C if per_cloud else 0, p(err), p(ws), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = table.cpu().numpy()
    assert (got[:4] == SENTINEL).all() and (got[4 + words:] == SENTINEL).all(), "the table's sentinels"
    assert (ws[nbytes // 4:].view(torch.int32) == GUARD).all(), "the workspace's guard words"
    shape = (B, C, 5) if per_cloud else (C, 5)
    return (got[4:4 + words] - held).reshape(shape), int(err.item())


def check(dev, case, per_cloud=False, **kw):
    """The device's table of ``case`` (``panoptic_table``'s keyword arguments) against the reference: equal int64, equal error bits."""
    arrays, begins, counts = layout(case)
    args = {k: case.get(k) for k in CALL}
    args["min_points"] = 30 if args["min_points"] is None else args["min_points"]
    got, err = call(dev, arrays, begins, counts, case["C"], per_cloud=per_cloud, **args, **kw)
    want, _, want_err = R.panoptic_table(case["pred_sem"], case["pred_inst"], case["gt_sem"], case["gt_inst"], case["C"],
                                         begins=case.get("begins"), counts=case.get("counts"), per_cloud=per_cloud, **args)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert err == want_err
    return got, err


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_row_counts_one_cloud(dev, n):
    case = R.random_case(n, n, C=5, segments=max(2, n // 20), ids=64)
    got, _ = check(dev, case)
    assert n < 64 or got[:, :3].sum() > 0
    check(dev, case, max_rows=n + 100)                               # a bound above the count changes nothing
    case = dict(case, things=None, include=None, min_points=1)
    check(dev, case)


def test_three_clouds_with_unequal_counts_one_of_them_empty(dev):
    case = R.random_case(7, 300, C=4, segments=15, B=3, ids=30)
    case["counts"] = [257, 0, 65]
    pooled, _ = check(dev, case)
    per, _ = check(dev, case, per_cloud=True)
    assert np.array_equal(per.sum(0), pooled) and not per[1].any() and per[0, :, 0].sum() > 0 and per[2, :, :3].sum() > 0
    # the same rows in every cloud: clouds never share segments
    one = R.random_case(8, 129, C=3, segments=6, ids=9)
    three = {k: (np.tile(v, 3) if k in ("pred_sem", "pred_inst", "gt_sem", "gt_inst") else v) for k, v in one.items()}
    three["begins"], three["counts"] = [0, 129, 258], [129, 129, 129]
    got, _ = check(dev, three)
    assert np.array_equal(got, 3 * check(dev, one)[0])
    # a count above max_rows is clamped: the rows beyond take no part
    arrays, begins, counts = layout(one)
    clamped, _ = call(dev, arrays, begins, [10 ** 9], 3, one["include"], one["things"], one["min_points"], max_rows=100)
    short = {k: (v[:100] if k in ("pred_sem", "pred_inst", "gt_sem", "gt_inst") else v) for k, v in one.items()}
    short["counts"] = [100]
    assert np.array_equal(clamped, check(dev, short)[0])
    negative, err = call(dev, arrays, begins, [-5], 3, one["include"], one["things"], one["min_points"], max_rows=100)
    assert not negative.any() and err == 0


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_worked_cases(dev, name):
    """The seams of the rule (tests/panoptic_ref.py, ``hand_cases``): the literal tables, not only the reference."""
    case = R.hand_cases()[name]
    got, err = check(dev, case)
    assert got.tolist() == case["table"].tolist() and err == case["err"]
    per, _ = check(dev, case, per_cloud=True)
    assert np.array_equal(per.sum(0), got)


def test_contention_and_spread(dev):
    n = 4099
    z = np.zeros(n, np.int64)
    one = {"pred_sem": z + 2, "pred_inst": z + 5, "gt_sem": z + 2, "gt_inst": z + 9, "C": 3}
    got, _ = check(dev, one)
    assert got.tolist() == [[0] * 5, [0] * 5, [1, 0, 0, 1 << 21, 0]]
    own = np.arange(257, dtype=np.int64)
    case = {"pred_sem": own * 0, "pred_inst": own + 1000, "gt_sem": own * 0, "gt_inst": own, "C": 1, "min_points": 1}
    got, _ = check(dev, case)
    assert got.tolist() == [[257, 0, 0, 257 << 21, 0]]
    case["pred_inst"] = np.where(own % 2 == 0, own, -1)              # every other row without a prediction
    got, _ = check(dev, case)
    assert got.tolist() == [[129, 0, 128, 129 << 21, 0]]
    assert check(dev, dict(case, min_points=2))[0].tolist() == [[129, 0, 0, 129 << 21, 0]]
    # 4 096 rows, each a segment and a pair of its own: all three tables at their fullest, half of the 8 192 slots
    full = np.arange(4096, dtype=np.int64)
    case = {"pred_sem": full * 0, "pred_inst": full * 3 + 7, "gt_sem": full * 0, "gt_inst": (full * 2654435761) % (1 << 31), "C": 1,
            "min_points": 1}
    assert check(dev, case)[0].tolist() == [[4096, 0, 0, 4096 << 21, 0]]
    mix = R.random_case(300, 9000, C=7, segments=300, ids=1 << 30, noise=0.05)
    got, _ = check(dev, mix)
    assert got[:, 0].sum() > 100 and got[:, 1].sum() > 20 and got[:, 2].sum() > 20


def test_order_and_accumulation(dev):
    case = R.random_case(41, 3000, C=6, segments=80, B=2, ids=500, noise=0.08)
    first, _ = check(dev, case, per_cloud=True)
    again, _ = check(dev, case, per_cloud=True)
    assert np.array_equal(first, again) and first[:, :, 0].sum() > 20
    rng = np.random.default_rng(5)
    perm = np.concatenate([rng.permutation(3000), 3000 + rng.permutation(3000)])         # inside each cloud
    shuffled = {k: (v[perm] if k in ("pred_sem", "pred_inst", "gt_sem", "gt_inst") else v) for k, v in case.items()}
    assert np.array_equal(check(dev, shuffled, per_cloud=True)[0], first)
    pooled, _ = check(dev, case)
    assert np.array_equal(first.sum(0), pooled)
    # two calls into one table: the sum of the two tables
    other = R.random_case(42, 2000, C=6, segments=50, ids=500)
    alone, _ = check(dev, other)
    out = torch.zeros(6, 5, dtype=torch.int64, device=dev)
    for c, shape in ((case, (2, 3000)), (other, (2000,))):
        metrics.panoptic_counts(*[t.view(shape) for t in device_case(c, dev)], 6, c["include"], c["things"], c["min_points"], out=out)
    assert np.array_equal(out.cpu().numpy(), pooled + alone) and alone[:, 0].sum() > 10


def test_captured_call_follows_the_device_side_counts(dev):
    cap, C = 4099, 5
    big, small = R.random_case(1, cap, C=C, segments=120, ids=999), R.random_case(2, 1500, C=C, segments=40, ids=999)
    ints = lambda: torch.zeros(2 * cap, dtype=torch.int32, device=dev)
    ps, pi, gs, gi = ints(), ints(), ints(), ints()
    begin = torch.tensor([0, cap], dtype=torch.int64, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    inc, th = mask(big["include"], dev), mask(big["things"], dev)
    out = torch.zeros(C, 5, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    work = metrics.panoptic_workspace(2, cap, dev)

    def load(first, second):
        for b, case in enumerate((first, second)):
            n = len(case["gt_sem"])
            for t, name in ((ps, "pred_sem"), (pi, "pred_inst"), (gs, "gt_sem"), (gi, "gt_inst")):
                t[b * cap:(b + 1) * cap] = 424242                    # rows beyond the count: poison
                t[b * cap:b * cap + n] = torch.from_numpy(case[name].astype(np.int32)).to(dev)
        count.copy_(torch.tensor([len(first["gt_sem"]), len(second["gt_sem"])]))

    def step():
        return metrics.panoptic_counts(ps, pi, gs, gi, C, inc, th, 3, begin, count, cap, out=out, err=err, work=work)

    def want(first, second):
        return sum(R.panoptic_table(c["pred_sem"], c["pred_inst"], c["gt_sem"], c["gt_inst"], C, c["include"], c["things"], 3)[0]
                   for c in (first, second))

    load(big, small)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and len(v) == 1500 else v) for k, v in small.items()}
    for first, second in ((small, big), (big, big), (empty, small)):
        load(first, second)
        out.zero_()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before               # nothing allocated by a replay
        replayed = out.cpu().numpy().copy()
        out.zero_()
        assert step() is out
        assert np.array_equal(out.cpu().numpy(), replayed) and np.array_equal(replayed, want(first, second))
    assert int(err.item()) == 0


def test_a_cloud_that_leaves_the_buffers_is_skipped_whole(dev):
    case = R.random_case(9, 200, C=3, segments=8, B=2, ids=20)
    arrays, begins, counts = layout(case)
    good, _ = call(dev, arrays, begins, counts, 3, case["include"], case["things"], case["min_points"], per_cloud=True)
    rows = len(arrays[0])
    for bad_begin in (-1, rows - 199, rows, 2 ** 40):
        got, err = call(dev, arrays, [begins[0], bad_begin], counts, 3, case["include"], case["things"], case["min_points"], per_cloud=True)
        assert err == R.ERR_ROWS and np.array_equal(got[0], good[0]) and not got[1].any()
    got, err = call(dev, arrays, [begins[0], rows - 200], counts, 3, case["include"], case["things"], case["min_points"], per_cloud=True)
    assert err == 0 and np.array_equal(got[0], good[0])              # the last cloud that still fits


def test_refusals_touch_nothing(dev):
    lib = _lib.load()
    n, C = 100, 3
    d = [torch.zeros(n + 1, dtype=torch.int32, device=dev) for _ in range(4)]
    begin, count = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), n, dtype=torch.int64, device=dev)
    inc = torch.ones(C + 1, dtype=torch.int32, device=dev)
    table = torch.full((C * 5 + 1,), SENTINEL, dtype=torch.int64, device=dev)
    nbytes = lib.pn2_panoptic_workspace_bytes(1, n)
    ws = torch.full((nbytes // 4 + 4,), float("nan"), dtype=torch.float32, device=dev)
    err = torch.full((2,), 77, dtype=torch.int32, device=dev)
    p = _lib.ptr
    good = dict(ps=p(d[0]), pi=p(d[1]), gs=p(d[2]), gi=p(d[3]), begin=p(begin), count=p(count), B=1, max_rows=n, rows=n, C=C, include=p(inc),
                things=None, min_points=30, table=p(table), stride=0, err=p(err), ws=p(ws))
    order = ("ps", "pi", "gs", "gi", "begin", "count", "B", "max_rows", "rows", "C", "include", "things", "min_points", "table", "stride",
             "err", "ws")
    bad = [{k: None} for k in ("ps", "pi", "gs", "gi", "begin", "count", "include", "table", "ws")]
    bad += [{"C": 0}, {"C": -1}, {"B": 0}, {"B": 65536}, {"max_rows": -1}, {"max_rows": _lib.VOXEL_MAX_ROWS + 1}, {"min_points": -1},
            {"rows": n - 1}, {"stride": 5 * C - 1}, {"stride": -1}]
    bad += [{k: good[k] + 2} for k in ("ps", "pi", "gs", "gi", "include", "err")]          # not 4-byte aligned
    bad += [{"things": p(inc) + 1}, {"begin": p(begin) + 4}, {"count": p(count) + 4}, {"table": p(table) + 4}, {"ws": p(ws) + 8}]
    for change in bad:
        args = dict(good, **change)
        assert lib.pn2_panoptic_count(*[args[k] for k in order], _lib.stream()) == -1, change
    torch.cuda.synchronize()
    assert (table == SENTINEL).all() and (err == 77).all() and torch.isnan(ws).all()
    assert lib.pn2_panoptic_count(*[good[k] for k in order], _lib.stream()) == 0          # the unchanged call is accepted
    torch.cuda.synchronize()
    assert int(err[0].item()) == 77 and table[:C * 5].tolist() == [SENTINEL + 1, SENTINEL, SENTINEL, SENTINEL + (1 << 21), SENTINEL] + \
        [SENTINEL] * 10                                              # (100 rows of class 0, id 0 on both sides: one match added)


# ------------------------------------------------------------------------------------------------------------- the Python layer
def device_case(case, dev):
    return [torch.from_numpy(np.asarray(case[k], np.int32)).to(dev) for k in ("pred_sem", "pred_inst", "gt_sem", "gt_inst")]


def test_panoptic_counts_input_shapes(dev):
    case = R.random_case(21, 600, C=4, segments=20, B=3, ids=50)
    kw = dict(include=case["include"], things=case["things"], min_points=case["min_points"])
    want, _, _ = R.panoptic_table(case["pred_sem"], case["pred_inst"], case["gt_sem"], case["gt_inst"], 4, begins=case["begins"],
                                  counts=case["counts"], per_cloud=True, **kw)
    flat = device_case(case, dev)
    got = metrics.panoptic_counts(*[t.view(3, 600) for t in flat], 4, per_cloud=True, **kw)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    got = metrics.panoptic_counts(*flat, 4, row_begin=t64(case["begins"]), row_count=t64(case["counts"]), max_rows=600, **kw)
    assert np.array_equal(got.cpu().numpy(), want.sum(0))
    one = metrics.panoptic_counts(*[t[:600].long() for t in flat], 4, **kw)                # any integer dtype, one cloud
    assert np.array_equal(one.cpu().numpy(), want[0])
    with pytest.raises(_lib.Pn2Error):
        metrics.panoptic_counts(*[t.cpu() for t in flat], 4)
    with pytest.raises(ValueError):
        metrics.panoptic_counts(*flat, 4, out=torch.zeros(4, 4, dtype=torch.int64, device=dev))


def test_evaluator_over_three_updates_and_the_scores(dev):
    C = 6
    cases = [R.random_case(60 + k, 2500 + 100 * k, C=C, segments=60, B=1 + k, ids=1 << 16, noise=0.03) for k in range(3)]
    inc, th = cases[0]["include"], cases[0]["things"]
    for per_cloud in (False, True):
        ev = metrics.PanopticEvaluator(C, include=inc, things=th, min_points=4, per_cloud=per_cloud, device=dev)
        want, fsum = [], np.zeros(C)
        for k, case in enumerate(cases):
            flat = device_case(case, dev)
            n = 2500 + 100 * k
            ev.update(*[t.view(1 + k, n) for t in flat])
            t, f, _ = R.panoptic_table(case["pred_sem"], case["pred_inst"], case["gt_sem"], case["gt_inst"], C, inc, th, 4,
                                       begins=case["begins"], counts=case["counts"], per_cloud=True)
            want.append(t)
            for b in range(1 + k):                                   # the API: one running sum, scan by scan
                fsum = fsum + f[b]
        want = np.concatenate(want, 0)
        tables = ev.tables()
        assert np.array_equal(tables, want if per_cloud else want.sum(0))
        ev.check()
        scores = ev.scores()
        total = want.sum(0)
        api = R.api_scores(total, fsum, inc)
        assert total[:, 0].sum() > 100
        assert scores["tp"].tolist() == total[:, 0].tolist() and scores["fp"].tolist() == total[:, 1].tolist()
        assert scores["fn"].tolist() == total[:, 2].tolist() and np.array_equal(scores["iou_sum"], R.iou_sum(total))
        assert np.array_equal(scores["rq_per_class"], api["rq_per_class"]) and scores["rq"] == api["rq"]       # integers only: exact
        # sq = sum / tp: the sums differ by at most tp * 2^-52 * sum (the stated deviation), each division rounds once (2^-53 relative)
        tp = np.maximum(total[:, 0], 1)
        sq_bound = R.deviation_bound(total) / tp + 2.0 ** -52 * scores["sq_per_class"]
        assert (np.abs(scores["sq_per_class"] - api["sq_per_class"]) <= sq_bound).all()
        pq_bound = sq_bound * scores["rq_per_class"] + 2.0 ** -52 * scores["pq_per_class"]
        assert (np.abs(scores["pq_per_class"] - api["pq_per_class"]) <= pq_bound).all()
        assert abs(scores["sq"] - api["sq"]) <= sq_bound.sum() and abs(scores["pq"] - api["pq"]) <= pq_bound.sum()
        assert 0 < scores["pq"] <= scores["sq"] <= 1 and 0 < scores["rq"] <= 1
    bad = metrics.PanopticEvaluator(C, device=dev)
    flat = device_case(cases[0], dev)
    flat[2][5] = C
    bad.update(*flat)
    with pytest.raises(KeyError):
        bad.check()


def test_update_scan_on_a_synthetic_scan_with_a_planted_prediction(dev):
    """What ``label_scan(..., instances=)`` leaves (raw ids, ``id + 1`` with 0 for none) against ``.label`` words."""
    rng = np.random.default_rng(77)
    M = 5000
    learning_map = {0: 0, 1: 0, 10: 1, 11: 2, 30: 3, 40: 4, 252: 1}     # raw id -> class; class 0 is ignored, 4 is stuff
    lut = np.full(253, -1, np.int32)
    for k, v in learning_map.items():
        lut[k] = v
    raw_ids = np.array(sorted(learning_map))
    runs = np.repeat(rng.integers(0, len(raw_ids), 100), 50)
    gt_raw, gt_inst = raw_ids[runs], np.repeat(rng.integers(0, 300, 100), 50)
    pred_raw, pred_plus1 = gt_raw.copy(), gt_inst + 1                # planted: the truth, then damaged
    flip = rng.random(M) < 0.1
    pred_raw[flip] = raw_ids[rng.integers(0, len(raw_ids), int(flip.sum()))]
    pred_plus1[rng.random(M) < 0.1] = 0                              # "no instance"
    pred_plus1[2000:2300] += 1000                                    # six segments under another id
    words = (gt_inst.astype(np.uint32) << np.uint32(16)) | gt_raw.astype(np.uint32)
    things, include = [0, 1, 1, 1, 0], [0, 1, 1, 1, 1]
    ev = metrics.PanopticEvaluator(5, include=include, things=things, min_points=5, device=dev)
    ev.update_scan(torch.from_numpy(pred_raw.astype(np.int32)).to(dev), torch.from_numpy(pred_plus1.astype(np.int32)).to(dev), words,
                   torch.from_numpy(lut).to(dev))
    want, _, _ = R.panoptic_table(lut[pred_raw], pred_plus1 - 1, lut[gt_raw], gt_inst, 5, include, things, 5)
    assert np.array_equal(ev.tables(), want) and want[:, 0].sum() > 20 and want[4, 0] == 1 and not want[0].any()
    ev.check()
    s, i = kitti.split_label_words(words, dev)
    assert s.is_cuda and np.array_equal(s.cpu().numpy(), gt_raw) and np.array_equal(i.cpu().numpy(), gt_inst)
    words[7] = 300                                                   # a raw id beyond the table: class -1, dropped, flagged
    ev.update_scan(torch.from_numpy(pred_raw.astype(np.int32)).to(dev), torch.from_numpy(pred_plus1.astype(np.int32)).to(dev), words,
                   torch.from_numpy(lut).to(dev))
    with pytest.raises(KeyError):
        ev.check()
