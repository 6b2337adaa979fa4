"""GPU: the device scan ingest (``pn2_scan_filter``, csrc/scan.hip; ``kitti.ScanFilter``) against ``kitti.read_scan`` -- the host
restatement of the reference's ``Semantic_KITTI_Utils.get`` -- on inputs where the two rules cannot differ, against the numpy
restatement of the device rule (tests/scan_filter_ref.py) at the borders, and through ``FrameSegmenter.frame_raw`` and
``load_scans(ingest="device")``.  Every call goes through the C ABI with poisoned output buffers (``run_abi``) and through the
Python class; every byte outside ``[out_begin[b], out_begin[b] + count[b])`` must come back untouched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scan_filter_ref as R
from conftest import golden
from pointnet12_amd import _lib, kitti
from pointnet12_amd import kitti_view as V

pytestmark = pytest.mark.gpu

T = _lib.SCAN_TILE
POISON_F, POISON_I = 0x5A5A5A5A, -777
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 131071, 128 * T + 1]     # (129 tiles: the scan's carry takes a third step)


def lmap_g9():
    g = golden("g9_kitti.npz")
    return {int(k): int(v) for k, v in zip(g["map_keys"], g["map_values"])}


def words_dev(words, dev):
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to(dev)


def run_abi(dev, raw, words, begins, counts, max_rows, lut, fov, box, out_begins=None, out_rows=None, labels=True, index=True):
    """One ``pn2_scan_filter`` call on host arrays: poisons the outputs, checks that nothing outside the kept ranges was written
    and returns ``(per-scan [(points, labels | None, index | None)], counts, err)`` as numpy (``labels`` of an unlabelled scan: zeros)."""
    lib = _lib.load()
    B = len(begins)
    out_begins = list(begins) if out_begins is None else list(out_begins)
    out_rows = len(raw) if out_rows is None else out_rows
    raw_d = torch.from_numpy(np.ascontiguousarray(raw, np.float32)).to(dev)
    lab_d = None if words is None else words_dev(words, dev)
    lut_d = None if lut is None else torch.from_numpy(np.ascontiguousarray(lut, np.int32)).to(dev)
    t64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)
    begin_d, count_d, ob_d = t64(begins), t64(counts), t64(out_begins)
    pts = torch.full((out_rows, 4), POISON_F, dtype=torch.int32, device=dev)
    lab = torch.full((out_rows,), POISON_I, dtype=torch.int32, device=dev)
    idx = torch.full((out_rows,), POISON_I, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -5, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = lib.pn2_scan_filter_workspace_bytes(B, max_rows)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    fp = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(ctypes.c_void_p)
    fov_a = None if fov is None else np.ascontiguousarray(fov, np.float32)
    box_a = None if box is None else np.ascontiguousarray(box, np.float32)
    p = _lib.ptr
    rc = lib.pn2_scan_filter(p(raw_d), p(lab_d), p(begin_d), p(count_d), B, max_rows, p(lut_d), 0 if lut is None else len(lut),
                             fp(fov_a), fp(box_a), p(ob_d), p(pts), p(lab) if labels else None, p(idx) if index else None, p(cnt),
                             p(err), p(ws), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    pts_h, lab_h, idx_h, cnt_h = pts.cpu().numpy(), lab.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()
    written = np.zeros(out_rows, bool)
    scans = []
    for b in range(B):
        lo, hi = out_begins[b], out_begins[b] + int(cnt_h[b])
        assert 0 <= cnt_h[b] <= max(0, min(counts[b], max_rows)) and hi <= out_rows and not written[lo:hi].any()
        written[lo:hi] = True
        scans.append((pts_h[lo:hi].view(np.float32), lab_h[lo:hi] if labels else None, idx_h[lo:hi] if index else None))
    assert (pts_h[~written].view(np.uint32) == POISON_F).all(), "out_points written outside the kept ranges"
    assert (lab_h[~written] == POISON_I).all() if labels else (lab_h == POISON_I).all(), "out_labels written outside the kept ranges"
    assert (idx_h[~written] == POISON_I).all() if index else (idx_h == POISON_I).all()
    return scans, cnt_h, int(err.item())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def check_against(ref, got, raw):
    """One scan's device result against a restatement / reference result dict (``points``, ``labels``, ``index``)."""
    pts, lab, idx = got
    assert len(pts) == len(ref["points"]) and same_bits(pts, ref["points"])
    if ref.get("labels") is not None and lab is not None:
        assert np.array_equal(lab, ref["labels"])
    if idx is not None:
        assert (np.diff(idx) > 0).all() and same_bits(raw[idx], pts)
        if ref.get("index") is not None:
            assert np.array_equal(idx, ref["index"])


@pytest.fixture(scope="module")
def decided():
    """One realistic decided scan (131 071 rows), its files' content and what ``kitti.read_scan`` returns for both subsets."""
    lmap = lmap_g9()
    pts, words = R.decided_scan(31, 131071, classes=sorted(lmap))
    return {"lmap": lmap, "lut": R.make_lut(lmap), "raw": pts, "words": words}


def host_read(tmp_path, raw, words, lmap, subset):
    fv, fl = os.path.join(tmp_path, "s.bin"), os.path.join(tmp_path, "s.label")
    raw.tofile(fv)
    words.tofile(fl)
    return kitti.read_scan(fv, fl, lmap, subset), (fv, fl)


@pytest.mark.parametrize("subset", ["inview", "all"])
def test_exact_on_decided_inputs(dev, tmp_path, decided, subset):
    raw, words, lmap, lut = decided["raw"], decided["words"], decided["lmap"], decided["lut"]
    (ref_pts, ref_lab), (fv, fl) = host_read(tmp_path, raw, words, lmap, subset)
    fov, box = (R.thresholds(), R.DEFAULT_BOX) if subset == "inview" else (None, None)
    rule = R.scan_filter(raw, words, lut, fov, box)
    assert same_bits(rule["points"], ref_pts) and 1000 < len(ref_pts) < len(raw)      # decided: the two host rules agree
    ref = {"points": ref_pts, "labels": ref_lab, "index": rule["index"]}
    scans, cnt, err = run_abi(dev, raw, words, [0], [len(raw)], len(raw), lut, fov, box)
    assert err == 0 and cnt[0] == len(ref_pts)
    check_against(ref, scans[0], raw)
    # the Python class, twice: byte-identical from run to run
    sf = kitti.ScanFilter(lmap, subset, device=dev)
    raw_d, lab_d = torch.from_numpy(raw).to(dev), words_dev(words, dev)
    runs = []
    for _ in range(2):
        p, l, i, c = sf.filter(raw_d, lab_d)
        assert c.dtype == torch.int64 and c.is_cuda and c.shape == (1,)
        m = int(c.item())
        runs.append((p[:m].cpu().numpy(), l[:m].cpu().numpy(), i[:m].cpu().numpy()))
        sf.check()
    check_against(ref, runs[0], raw)
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(runs[0], runs[1]))
    dp, dl = kitti.read_scan_device(fv, fl, sf)
    assert dp.shape == ref_pts.shape and same_bits(dp.cpu().numpy(), ref_pts) and np.array_equal(dl.cpu().numpy(), ref_lab)
    assert dl.dtype == torch.int32


@pytest.mark.parametrize("M", SIZES)
def test_compaction_sizes_and_patterns(dev, M):
    """The keep pattern comes from the class word (lut: 0 -> dropped, 1 -> class 0), no geometric test: all kept, none kept,
    alternating, and kept only in the last wave of the last tile."""
    rng = np.random.default_rng(M)
    raw = rng.normal(size=(M, 4)).astype(np.float32)
    lut = np.array([0, 1, 5], np.int32)
    last_wave = np.zeros(M, bool)
    last_wave[(M - 1) // 64 * 64:] = True
    patterns = {"all": np.ones(M, bool), "none": np.zeros(M, bool), "alternating": np.arange(M) % 2 == 1, "last_wave": last_wave}
    sf = kitti.ScanFilter({0: 0, 1: 1, 2: 5}, "all", device=dev)
    for name, keep in patterns.items():
        words = np.where(keep, np.where(np.arange(M) % 3 == 0, 2, 1), 0).astype(np.uint32) | np.uint32(0x00070000)
        ref = R.scan_filter(raw, words, lut)
        assert np.array_equal(ref["mask"], keep)
        scans, cnt, err = run_abi(dev, raw, words, [0], [M], M, lut, None, None)
        assert err == 0 and cnt[0] == keep.sum(), name
        check_against(ref, scans[0], raw)
        p, l, i, c = sf.filter(torch.from_numpy(raw).to(dev), words_dev(words, dev))
        m = int(c.item())
        assert m == keep.sum(), name
        check_against(ref, (p[:m].cpu().numpy(), l[:m].cpu().numpy(), i[:m].cpu().numpy()), raw)


def test_batched_ragged(dev):
    lmap = lmap_g9()
    lut = R.make_lut(lmap)
    counts = [T + 5, 0, 200]
    begins = [3, T + 20, T + 20]
    rows = T + 20 + 200 + 9
    raw, words = R.decided_scan(7, rows, classes=sorted(lmap))
    fov, box = R.thresholds(), R.DEFAULT_BOX
    refs = [R.scan_filter(raw[b:b + c], words[b:b + c], lut, fov, box) for b, c in zip(begins, counts)]
    out_begins = [11, 5, T + 40]
    scans, cnt, err = run_abi(dev, raw, words, begins, counts, T + 5, lut, fov, box, out_begins, out_rows=T + 40 + 200 + 3)
    assert err == 0 and cnt.tolist() == [len(r["points"]) for r in refs] and cnt[1] == 0 and cnt[0] > 0 and cnt[2] > 0
    for b in range(3):
        check_against(refs[b], scans[b], raw[begins[b]:begins[b] + counts[b]])
    # through the class, outputs at row_begin
    sf = kitti.ScanFilter(lmap, device=dev)
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    p, l, i, c = sf.filter(torch.from_numpy(raw).to(dev), words_dev(words, dev), t64(begins), t64(counts), T + 5)
    c = c.cpu().tolist()
    assert c == cnt.tolist() and int(sf.error_flag.item()) == 0
    for b in range(3):
        lo, hi = begins[b], begins[b] + c[b]
        check_against(refs[b], (p[lo:hi].cpu().numpy(), l[lo:hi].cpu().numpy(), i[lo:hi].cpu().numpy()), raw[begins[b]:begins[b] + counts[b]])
    # a row_count above max_rows: its bit is set and the rows beyond max_rows are ignored
    short = R.scan_filter(raw[3:3 + T], words[3:3 + T], lut, fov, box)
    scans, cnt, err = run_abi(dev, raw, words, begins, counts, T, lut, fov, box, out_begins, out_rows=T + 40 + 200 + 3)
    assert err == _lib.SCAN_ERR_ROWS and cnt.tolist() == [len(short["points"]), 0, len(refs[2]["points"])]
    check_against(short, scans[0], raw[3:3 + T])
    check_against(refs[2], scans[2], raw[begins[2]:begins[2] + 200])
    sf.filter(torch.from_numpy(raw).to(dev), words_dev(words, dev), t64(begins), t64(counts), T)
    with pytest.raises(ValueError):
        sf.check()


@pytest.mark.parametrize("name", ["az_lo", "az_hi", "el_lo", "el_hi"])
def test_borders(dev, name):
    pts, _ = R.sweeps()[name]
    fov, box = R.thresholds(), R.DEFAULT_BOX
    ref = R.scan_filter(pts, None, None, fov, box, w=1)
    band = ref["undecided"]
    assert 0 < band.sum() <= 0.01 * len(pts)
    scans, cnt, err = run_abi(dev, pts, None, [0], [len(pts)], len(pts), None, fov, box)
    got_pts, got_lab, got_idx = scans[0]
    assert err == 0 and not got_lab.any()                             # (an unlabelled scan's classes are zeros)
    mask = np.zeros(len(pts), bool)
    mask[got_idx] = True
    differ = mask != ref["mask"]
    print("sweep %s: %d kept, %d in the w = 1 band, %d differ, %d outside the band"
          % (name, mask.sum(), band.sum(), differ.sum(), (differ & ~band).sum()))
    assert not (differ & ~band).any()
    # inside the band a point may go either way, but the outputs agree with one another
    assert cnt[0] == mask.sum() == len(got_idx) and (np.diff(got_idx) > 0).all() and same_bits(got_pts, pts[got_idx])


@pytest.mark.parametrize("subset", ["all", "inview"])
def test_recorded_scan_through_the_device(dev, subset):
    g = golden("g9_kitti.npz")
    lmap = lmap_g9()
    lut = R.make_lut(lmap)
    raw, words = np.ascontiguousarray(g["bin"]), np.ascontiguousarray(g["label"])
    rec = R.recorded_mask(raw, words, g[subset + "/points"], g[subset + "/labels"], lut)
    fov, box = (R.thresholds(), R.DEFAULT_BOX) if subset == "inview" else (None, None)
    und = R.undecided(raw, R.thresholds(), 4) if subset == "inview" else np.zeros(len(raw), bool)
    assert und.sum() <= 2
    scans, cnt, err = run_abi(dev, raw, words, [0], [len(raw)], len(raw), lut, fov, box)
    pts, lab, idx = scans[0]
    mask = np.zeros(len(raw), bool)
    mask[idx] = True
    print("g9 %s on the device: %d kept, %d undecided at w = 4, %d differ from the recorded output" % (subset, cnt[0], und.sum(), (mask != rec).sum()))
    assert err == 0 and not ((mask != rec) & ~und).any()
    assert same_bits(pts, raw[idx]) and np.array_equal(lab, (lut[words[idx] & 0xFFFF] - 1).astype(np.int32))
    if not (mask != rec).any():
        assert same_bits(pts, g[subset + "/points"]) and np.array_equal(lab, g[subset + "/labels"])


def test_special_values(dev):
    inf, nan = np.inf, np.nan
    rows = [[5, 0, 0, 0.1], [0, 0, 0, 0.2], [-0.0, 0.0, 0, 0.3], [0.0, -0.0, 0, 0.4], [5, 1, 0.5, 0.5]]
    for k in range(3):
        for v in (nan, inf, -inf):
            r = [5.0, 1.0, 0.5, 0.6]
            r[k] = v
            rows.append(r)
    rows += [[3e19, 1.0, 0.0, 0.7], [6, -1, 0.2, nan]]               # d overflows float32; a NaN intensity is no coordinate
    pts = np.array(rows, np.float32)
    fov = R.thresholds()
    for box in (R.DEFAULT_BOX, (-3e38, 3e38) * 4):
        ref = R.scan_filter(pts, None, None, fov, box)
        assert ref["mask"].tolist() == [True, True, False, True, True] + [False] * 9 + [False, True]
        scans, cnt, err = run_abi(dev, pts, None, [0], [len(pts)], len(pts), None, fov, box)
        assert err == 0 and np.array_equal(scans[0][2], ref["index"])
        assert np.array_equal(scans[0][0].view(np.uint32), ref["points"].view(np.uint32))       # (NaN intensity: compared as bits)
    # without any geometric test every row passes, NaN rows included, as in the reference's subset 'all'
    scans, cnt, err = run_abi(dev, pts, None, [0], [len(pts)], len(pts), None, None, None)
    assert cnt[0] == len(pts) and np.array_equal(scans[0][0].view(np.uint32), pts.view(np.uint32))
    # classes: lut_len = 6; class 7 lies beyond it, class 2 maps to -1: both dropped, both reported; instance bits are ignored
    lut = R.make_lut({0: 0, 1: 1, 5: 3})
    good = np.tile(np.array([[5, 0, 0, 0.5]], np.float32), (6, 1))
    for words, keep, labels, bit in (([1, 0, 5, (0xABCD << 16) | 5, (0xFFFF << 16) | 0, 1], [0, 2, 3, 5], [0, 2, 2, 0], 0),
                                     ([1, 7, 5, 1, 1, 1], [0, 2, 3, 4, 5], [0, 2, 0, 0, 0], _lib.SCAN_ERR_CLASS),
                                     ([1, 2, 5, 1, 1, 1], [0, 2, 3, 4, 5], [0, 2, 0, 0, 0], _lib.SCAN_ERR_CLASS),
                                     ([1, (3 << 16) | 0xFFFF, 5, 1, 1, 1], [0, 2, 3, 4, 5], [0, 2, 0, 0, 0], _lib.SCAN_ERR_CLASS)):
        scans, cnt, err = run_abi(dev, good, np.array(words, np.uint32), [0], [6], 6, lut, fov, R.DEFAULT_BOX)
        assert err == bit and scans[0][2].tolist() == keep and scans[0][1].tolist() == labels
    sf = kitti.ScanFilter({0: 0, 1: 1, 5: 3}, device=dev)
    sf.filter(torch.from_numpy(good).to(dev), words_dev(np.array([1, 2, 5, 1, 1, 1], np.uint32), dev))
    with pytest.raises(KeyError):
        sf.check()


def test_unlabelled_scans(dev, decided):
    raw = decided["raw"][:3 * T + 17]
    fov, box = R.thresholds(), R.DEFAULT_BOX
    ref = R.scan_filter(raw, None, None, fov, box)
    for labels, index in ((True, True), (False, True), (False, False)):
        scans, cnt, err = run_abi(dev, raw, None, [0], [len(raw)], len(raw), None, fov, box, labels=labels, index=index)
        assert err == 0 and cnt[0] == ref["mask"].sum() and same_bits(scans[0][0], ref["points"])
    sf = kitti.ScanFilter(None, device=dev)
    p, l, i, c = sf.filter(torch.from_numpy(raw).to(dev))
    m = int(c.item())
    assert l is None and m == ref["mask"].sum() and same_bits(p[:m].cpu().numpy(), ref["points"])
    assert np.array_equal(i[:m].cpu().numpy(), ref["index"])
    with pytest.raises(ValueError):
        sf.filter(torch.from_numpy(raw).to(dev), words_dev(decided["words"][:len(raw)], dev))      # labels, but no map


def test_capture_and_replay_with_another_count(dev, decided):
    """``filter(out=...)`` + the device choice + ``pn2_prepare_clouds`` as one captured chain on one stream; replayed after a
    scan with another count has been copied into the static input, it gives the eager bytes."""
    lib = _lib.load()
    lmap, cap, n = decided["lmap"], 3 * T + 17, 512
    scan_a = (decided["raw"][:cap], decided["words"][:cap])
    scan_b = (decided["raw"][cap:cap + 2 * T + 3], decided["words"][cap:cap + 2 * T + 3])
    sf = kitti.ScanFilter(lmap, device=dev)
    bufs = sf.buffers(cap)
    raw_s = torch.zeros(cap, 4, device=dev)
    words_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    begin = torch.zeros(1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    u = torch.rand(n, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    normed = torch.zeros(1, n, 4, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    p = _lib.ptr

    def load(scan):
        m = len(scan[0])
        raw_s[:m].copy_(torch.from_numpy(scan[0]))
        words_s[:m].copy_(words_dev(scan[1], dev))
        count.fill_(m)

    def step():
        pts, lab, idx, kept = sf.filter(raw_s, words_s, begin, count, cap, out=bufs)
        choice = torch.minimum((u * kept).long(), kept - 1)
        assert lib.pn2_prepare_clouds(p(pts), p(begin), p(kept), None, None, None, p(choice), 1, n, p(normed), None, p(flag),
                                      _lib.stream()) == 0
        return choice

    def snapshot(choice):
        torch.cuda.synchronize()
        m = int(bufs.count.item())
        return (m, bufs.points[:m].clone(), bufs.labels[:m].clone(), bufs.index[:m].clone(), choice.clone(), normed.clone(), int(flag.item()))

    load(scan_a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured_choice = step()
    load(scan_b)
    graph.replay()
    replayed = snapshot(captured_choice)
    normed.zero_()
    bufs.count.zero_()
    eager = snapshot(step())
    ref = R.scan_filter(scan_b[0], scan_b[1], decided["lut"], R.thresholds(), R.DEFAULT_BOX)
    assert replayed[0] == eager[0] == ref["mask"].sum() and 0 < replayed[0] < len(scan_b[0])
    assert replayed[6] == eager[6] == 0
    for a, b in zip(replayed[1:6], eager[1:6]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert same_bits(replayed[1].cpu().numpy(), ref["points"]) and int(replayed[4].max()) < replayed[0]


class Stub(torch.nn.Module):
    """A tiny stand-in for the network: ``[1, 4, n]`` -> log-probabilities ``[1, n, 19]``."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(4, 19, generator=torch.Generator().manual_seed(0)))

    def forward(self, x):
        return torch.log_softmax(x.transpose(2, 1) @ self.w, -1)


def test_frame_raw(dev, tmp_path, decided, monkeypatch):
    g = golden("g18_kitti_view.npz")
    lmap = decided["lmap"]
    raw, words = decided["raw"][:5000], decided["words"][:5000]
    (host_pts, host_lab), _ = host_read(tmp_path, raw, words, lmap, "inview")
    n = 1024
    seg = V.FrameSegmenter(Stub().to(dev), V.Calibration(g["R"], g["T"], g["P"]), g["colors"], npoints=n)
    sf = kitti.ScanFilter(lmap, device=dev)
    choice = np.random.default_rng(5).integers(0, len(host_pts), n)
    a = seg.frame(host_pts, choice=choice)
    image_a, pred_a = a["image"].clone(), a["pred"].clone()
    b = seg.frame_raw(raw, words, scan_filter=sf, choice=choice)
    assert int(b["count"].item()) == len(host_pts) and int(seg.error_flag.item()) == 0 and int(sf.error_flag.item()) == 0
    assert torch.equal(b["image"], image_a) and torch.equal(b["pred"], pred_a) and image_a.any()
    assert np.array_equal(b["labels"][:len(host_lab)].cpu().numpy(), host_lab)
    # rng="numpy": the one count is read back, the draw is numpy's
    np.random.seed(9)
    c = seg.frame_raw(raw, words, scan_filter=sf)
    np.random.seed(9)
    expect = host_pts[np.random.choice(len(host_pts), n, replace=True)]
    assert same_bits(c["pts_3d"].cpu().numpy(), expect[:, :3])
    # a device generator and device inputs: nothing is read back (no .item() / .cpu() / synchronize is reached)
    raw_d, words_d = torch.from_numpy(raw).to(dev), words_dev(words, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    sf_live = kitti.ScanFilter(None, device=dev)                     # a live feed: no labels, no class map
    seg.frame_raw(raw_d, None, scan_filter=sf_live, rng=gen)
    seg.frame_raw(raw_d, words_d, scan_filter=sf, rng=gen)           # (buffers exist, kernels are loaded)
    torch.cuda.synchronize()

    def forbidden(*args, **kwargs):
        raise AssertionError("frame_raw read something back")
    with monkeypatch.context() as mp:
        for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "nonzero"):
            mp.setattr(torch.Tensor, name, forbidden)
        mp.setattr(torch.cuda, "synchronize", forbidden)
        d = seg.frame_raw(raw_d, words_d, scan_filter=sf, rng=gen)
        count_d = d["count"].clone()
        e = seg.frame_raw(raw_d, None, scan_filter=sf_live, rng=gen)
    torch.cuda.synchronize()
    assert int(seg.error_flag.item()) == 0 and e["labels"] is None and int(e["count"].item()) >= int(count_d.item()) > 0
    picked = e["pts_3d"].cpu().numpy()
    rows = {r.tobytes() for r in raw[:, :3]}
    assert all(r.tobytes() in rows for r in picked[:64])
    # nothing survives: the device choice is -1 and pn2_prepare_clouds flags it
    behind = raw.copy()
    behind[:, 0] = -np.abs(behind[:, 0]) - 1
    f = seg.frame_raw(behind, words, scan_filter=sf, rng=gen)
    assert int(f["count"].item()) == 0 and int(seg.error_flag.item()) != 0
    with pytest.raises(ValueError):
        seg.frame_raw(behind, words, scan_filter=sf)


def test_load_scans_device_ingest(dev, tmp_path, decided):
    lmap = decided["lmap"]
    pairs, at = [], 0
    for k, m in enumerate((T + 7, 0, 3000, 517)):
        fv, fl = os.path.join(tmp_path, "%06d.bin" % k), os.path.join(tmp_path, "%06d.label" % k)
        decided["raw"][at:at + m].tofile(fv)
        decided["words"][at:at + m].tofile(fl)
        pairs.append((fv, fl))
        at += m
    for subset in ("inview", "all"):
        host = kitti.load_scans(pairs, lmap, subset, device=dev)
        for chunk_rows in (1 << 22, 2000):                           # one chunk; three chunks
            store = kitti.load_scans(pairs, lmap, subset, device=dev, ingest="device", chunk_rows=chunk_rows)
            assert torch.equal(store.row_count, host.row_count) and torch.equal(store.row_begin, host.row_begin)
            assert torch.equal(store.raw.view(torch.int32), host.raw.view(torch.int32)) and torch.equal(store.label, host.label)
            assert store.label.dtype == torch.int32 and torch.equal(store._count_dev.cpu(), host.row_count)
    with pytest.raises(ValueError):
        kitti.load_scans(pairs, lmap, ingest="gpu")
