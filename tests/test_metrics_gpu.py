"""GPU: device-side segmentation metrics (pointnet12_amd/metrics.py on pn2_seg_confusion, csrc/metrics.hip).

Everything here is integer counting, so everything is held EXACTLY: the tables and predictions of the recorded cases
(tests/golden/g16_metrics.npz, tools/make_golden_metrics.py), of large generated cases against torch.bincount on the CPU copies,
through padded slices, with ignore_index, accumulated, replayed from a captured graph.  The reference-named functions are held
bit for bit against tests/metrics_ref.py (itself held against the reference by tests/test_metrics_cpu.py) and against the numbers
the reference's own loops returned; only name-grouped means get 4 ulp (pandas sums groups with compensation)."""
import numpy as np
import pytest
import torch

from conftest import golden
import metrics_ref as R

from pointnet12_amd import metrics as M

pytestmark = pytest.mark.gpu

CASES = ("s13", "k20", "p50", "ties", "special", "c1", "clf")


def G():
    return golden("g16_metrics.npz")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def case(g, c, dev):
    return torch.from_numpy(g[c + "/logp"]).to(dev), torch.from_numpy(g[c + "/target"]).to(dev)


def batch_tables(g, c, per_cloud):
    parts = np.split(g[c + "/tables"], int(g[c + "/nbatch"]))
    return parts if per_cloud else [p.sum(0) for p in parts]


def batch_points(g, c):
    B, N = g[c + "/target"].shape
    return [B // int(g[c + "/nbatch"]) * N] * int(g[c + "/nbatch"])


def same(t, a):
    return t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), a)


def test_golden_cases_pooled_and_per_cloud(dev):
    g = G()
    for c in CASES:
        lp, tg = case(g, c, dev)
        B, N, C = lp.shape
        conf, pred = M.confusion(lp, tg, per_cloud=True, return_pred=True)
        assert conf.shape == (B, C + 1, C) and same(conf, g[c + "/tables"]), c
        assert pred.shape == tg.shape and same(pred, g[c + "/pred"]), c
        pooled = M.confusion(lp, tg, C)
        assert pooled.shape == (C + 1, C) and same(pooled, g[c + "/tables"].sum(0)), c
        flat, fpred = M.confusion(lp.reshape(B * N, C), tg.reshape(-1), return_pred=True)                  # [R, C]: one cloud
        assert same(flat, g[c + "/tables"].sum(0)) and fpred.shape == (B * N,) and same(fpred, g[c + "/pred"].reshape(-1)), c
        assert same(M.confusion(lp, tg[:, :, None], per_cloud=True), g[c + "/tables"]), c                   # [B, N, 1] labels
        I, U = M.iou_counts(conf)
        for b in range(B):
            ri, ru = R.iou_counts(g[c + "/tables"][b])
            assert same(I[b], ri) and same(U[b], ru), c
    lp, tg = case(g, "s13", dev)
    for dtype in (torch.int32, torch.int16, torch.uint8, torch.int8):
        assert same(M.confusion(lp, tg.to(dtype), per_cloud=True), g["s13/tables"]), dtype
    lp, tg = case(g, "special", dev)                            # 255 as a uint8 label is still no class; so is -1 as int8
    t8 = torch.where((tg >= 0) & (tg < 13), tg, torch.full_like(tg, 255)).to(torch.uint8)
    assert same(M.confusion(lp, t8, per_cloud=True), g["special/tables"])
    with pytest.raises(RuntimeError):
        M.confusion(lp.double(), tg)
    with pytest.raises(RuntimeError):
        M.confusion(lp, tg.float())


def padded(lp, ld, fill, shift=0):
    """The same rows as a column slice of a [B*N, ld] buffer whose other columns hold `fill` values (NaN, +inf alternating);
    shift = 1 moves the buffer off its 16-byte alignment."""
    B, N, C = lp.shape
    store = torch.empty(B * N * ld + shift, device=lp.device, dtype=torch.float32)
    buf = store[shift:].view(B * N, ld)
    buf[:, 0::2] = fill[0]
    buf[:, 1::2] = fill[1]
    buf[:, :C] = lp.reshape(B * N, C)
    view = buf[:, :C].view(B, N, C) if ld == C else buf.view(B, N, ld)[:, :, :C]
    assert view.data_ptr() == buf.data_ptr() and view.stride(-2) == ld
    return view


def test_padded_slices_are_read_in_place_and_their_pad_never_counts(dev):
    g = G()
    nan, inf = float("nan"), float("inf")
    for c in CASES:
        lp, tg = case(g, c, dev)
        C = lp.shape[-1]
        for ld, shift in (((C + 3) & ~3, 0), (C + 3, 0), ((C + 3) & ~3, 1), (C + 5, 1)):
            for fill in ((nan, inf), (inf, nan)):
                view = padded(lp, ld, fill, shift)
                read, B, N, pitch = M._rows(view, C)
                assert read.data_ptr() == view.data_ptr() and pitch == ld and (B, N) == tuple(lp.shape[:2])       # no copy
                conf, pred = M.confusion(view, tg, per_cloud=True, return_pred=True)
                assert same(conf, g[c + "/tables"]) and same(pred, g[c + "/pred"]), (c, ld, shift, fill)
                assert same(M.confusion(view, tg), g[c + "/tables"].sum(0)), (c, ld, shift, fill)
                flat = view.as_strided((B * N, C), (ld, 1))                                                  # the same rows as [R, C]
                assert flat.data_ptr() == view.data_ptr()
                assert same(M.confusion(flat, tg.reshape(-1)), g[c + "/tables"].sum(0)), (c, ld, shift, fill)
    # num_classes below the width of the tensor: the columns beyond are pad too
    lp, tg = case(g, "s13", dev)
    wide = padded(lp, 16, (inf, nan))
    whole = wide.as_strided((3, 1024, 16), wide.stride())
    assert same(M.confusion(whole, tg, 13, per_cloud=True), g["s13/tables"])


def test_ignore_index(dev):
    g = G()
    for c, ignore in (("s13", None), ("k20", None), ("p50", None), ("special", 255), ("special", -1), ("special", 13), ("c1", 1),
                      ("ties", 6), ("clf", None), ("s13", -100)):
        lp, tg = case(g, c, dev)
        C = lp.shape[-1]
        if ignore is None:
            ignore = int(g[c + "/target"][0, 0])                                   # a label the case does hold
        want = R.count_tables(g[c + "/pred"], g[c + "/target"], C, ignore)
        if ignore != -100:
            assert want.sum() < g[c + "/target"].size, (c, ignore)
        conf, pred = M.confusion(lp, tg, per_cloud=True, ignore_index=ignore, return_pred=True)
        assert same(conf, want) and same(pred, g[c + "/pred"]), (c, ignore)                # ignored rows are still predicted
        assert same(M.confusion(padded(lp, C + 3, (float("nan"), float("inf"))), tg, ignore_index=ignore), want.sum(0)), (c, ignore)


def generated(seed, B, N, C, strays=True):
    """CPU tensors: log-probabilities of random logits that favour the label, labels in runs (a scanned surface), a few labels
    that are no class.  Expected tables by torch.bincount over (label row, CPU arg-max)."""
    gen = torch.Generator().manual_seed(seed)
    runs = torch.randint(0, C, (B, (N + 15) // 16), generator=gen)
    target = runs.repeat_interleave(16, dim=1)[:, :N].contiguous()
    logits = torch.randn(B, N, C, generator=gen)
    logits.scatter_add_(2, target[:, :, None], torch.full((B, N, 1), 1.5))
    lp = torch.log_softmax(logits, -1)
    if strays:
        where = torch.randint(0, N, (B, 64), generator=gen)
        target.scatter_(1, where, torch.tensor([-1, C, 255, -100]).repeat(B, 16))
    return lp, target


def expected(lp, target, C, per_cloud):
    B, N = target.shape
    pred = lp[..., :C].argmax(-1)
    row = torch.where((target >= 0) & (target < C), target, torch.full_like(target, C))
    cloud = torch.arange(B)[:, None].expand(B, N) if per_cloud else torch.zeros(B, N, dtype=torch.int64)
    flat = (cloud * (C + 1) + row) * C + pred
    nb = B if per_cloud else 1
    return torch.bincount(flat.reshape(-1), minlength=nb * (C + 1) * C).view(*((nb, C + 1, C) if per_cloud else (C + 1, C))), pred


@pytest.mark.parametrize("B,N,C", [(16, 4096, 13), (4, 100000, 20), (16, 2048, 50)])
def test_large_cases_equal_bincount_on_the_cpu_copies(dev, B, N, C):
    lp, target = generated(B * 1000 + C, B, N, C)
    want_pc, want_pred = expected(lp, target, C, True)
    want_pool, _ = expected(lp, target, C, False)
    assert int(want_pc[:, C].sum()) > 0 and int(want_pool.sum()) == B * N
    d_lp, d_t = lp.to(dev), target.to(dev)
    conf, pred = M.confusion(d_lp, d_t, per_cloud=True, return_pred=True)
    assert torch.equal(conf.cpu(), want_pc) and torch.equal(pred.cpu(), want_pred)
    assert torch.equal(M.confusion(d_lp, d_t).cpu(), want_pool)
    view = padded(d_lp, (C + 3) & ~3 if C % 4 else C + 4, (float("nan"), float("inf")))
    assert torch.equal(M.confusion(view, d_t, per_cloud=True).cpu(), want_pc)
    assert torch.equal(M.confusion(padded(d_lp, C + 1, (float("inf"), float("nan"))), d_t).cpu(), want_pool)


def test_every_row_of_a_cloud_in_one_bin(dev):
    """Maximal contention: all 65 536 rows of a cloud carry the same label and the same prediction."""
    B, N, C = 4, 65536, 13
    lp = torch.full((B, N, C), -5.0)
    target = torch.empty(B, N, dtype=torch.int64)
    for b in range(B):
        lp[b, :, (b + 1) % C] = 0.0
        target[b] = b if b < 3 else C + 7
    want_pc, want_pred = expected(lp, target, C, True)
    assert int((want_pc != 0).sum()) == B and int(want_pc.max()) == N
    conf, pred = M.confusion(lp.to(dev), target.to(dev), per_cloud=True, return_pred=True)
    assert torch.equal(conf.cpu(), want_pc) and torch.equal(pred.cpu(), want_pred)
    lp[:] = lp[0]
    target[:] = 0
    pooled = M.confusion(lp.to(dev), target.to(dev)).cpu()
    assert int(pooled[0, 1]) == B * N and int(pooled.sum()) == B * N


def test_accumulation_into_out_and_run_to_run_identity(dev):
    lp1, t1 = generated(1, 8, 4096, 13)
    lp2, t2 = generated(2, 8, 4096, 13)
    w1, _ = expected(lp1, t1, 13, True)
    w2, _ = expected(lp2, t2, 13, True)
    d1, d2 = (lp1.to(dev), t1.to(dev)), (lp2.to(dev), t2.to(dev))
    out = torch.zeros(8, 14, 13, device=dev, dtype=torch.int64)
    assert M.confusion(*d1, per_cloud=True, out=out) is out
    M.confusion(*d2, per_cloud=True, out=out)
    assert torch.equal(out.cpu(), w1 + w2)
    pooled = torch.zeros(14, 13, device=dev, dtype=torch.int64)
    for _ in range(3):
        M.confusion(*d1, out=pooled)
    assert torch.equal(pooled.cpu(), 3 * w1.sum(0))
    runs = [M.confusion(*d2, per_cloud=True).cpu() for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], w2)
    with pytest.raises(ValueError):
        M.confusion(*d1, per_cloud=True, out=pooled)
    # the evaluator's tape: more updates than its first allocation holds, one read at the end
    ev = M.SegEvaluator(13, per_cloud=True)
    for i in range(9):
        ev.update(*(d1 if i % 2 == 0 else d2))
    tables = ev.tables()
    assert tables.shape == (72, 14, 13) and tables.dtype == np.int64 and len(ev) == 72
    for i in range(9):
        assert np.array_equal(tables[8 * i:8 * i + 8], (w1 if i % 2 == 0 else w2).numpy()), i
    assert ev.batches[3] == (24, 8, 8 * 4096)
    ev = M.SegEvaluator(13)
    for i in range(40):
        ev.update(*(d1 if i % 3 else d2))
    tables = ev.tables()
    assert tables.shape == (40, 14, 13)
    for i in range(40):
        assert np.array_equal(tables[i], (w1 if i % 3 else w2).sum(0).numpy()), i
    assert M.SegEvaluator(13).tables().shape == (0, 14, 13)


def test_confusion_is_capturable(dev):
    """confusion(..., out=static) inside torch.cuda.graph, replayed on fresh data three times: the sum of the three tables.  A
    hidden synchronisation or read-back would fail the capture."""
    data = [generated(10 + i, 4, 8192, 20) for i in range(3)]
    s_lp, s_t = torch.zeros(4, 8192, 20, device=dev), torch.zeros(4, 8192, dtype=torch.int64, device=dev)
    s_out = torch.zeros(4, 21, 20, device=dev, dtype=torch.int64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.confusion(s_lp, s_t, per_cloud=True, out=s_out)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.confusion(s_lp, s_t, per_cloud=True, out=s_out)
    s_out.zero_()
    want = torch.zeros(4, 21, 20, dtype=torch.int64)
    for lp, t in data:
        s_lp.copy_(lp)
        s_t.copy_(t)
        graph.replay()
        want += expected(lp, t, 20, True)[0]
    torch.cuda.synchronize()
    assert torch.equal(s_out.cpu(), want)


class Stub:
    """A 'model' that hands out recorded log-probabilities batch by batch (on the device), wrapped as each family returns them."""

    def __init__(self, batches, dev, wrap=lambda lp: lp):
        self.batches, self.dev, self.wrap, self.i, self.args = batches, dev, wrap, 0, []

    def eval(self):
        return self

    def __call__(self, *args):
        assert all(a.is_cuda for a in args) and not torch.is_grad_enabled()
        self.args.append([tuple(a.shape) for a in args])
        lp = torch.from_numpy(self.batches[self.i]).to(self.dev)
        self.i += 1
        return self.wrap(lp)


def batches_of(g, c):
    n = int(g[c + "/nbatch"])
    return np.split(g[c + "/logp"], n), np.split(g[c + "/target"], n)


def test_calc_categorical_iou_and_compute_cat_iou(dev):
    g = G()
    for c in CASES:
        C = g[c + "/logp"].shape[-1]
        calc, cat, lst = np.zeros((C, 3)), np.zeros((C, 3)), []
        for lp, tg in zip(*batches_of(g, c)):
            d_lp = torch.from_numpy(lp).to(dev)
            t3 = torch.from_numpy(tg.copy()).to(dev)[:, :, None]
            calc = M.calc_categorical_iou(d_lp, t3, C, calc)
            assert t3.dim() == 2 or tg.shape[1] == 1                         # the reference squeezes its argument in place
            cat, more = M.compute_cat_iou(d_lp, torch.from_numpy(tg.copy()).to(dev), C, cat)
            lst += more
        assert np.array_equal(bits(calc[:, :2]), bits(g[c + "/calc_tabel"])) and not calc[:, 2].any(), c     # the reference's own numbers
        assert np.array_equal(bits(cat[:, :2]), bits(g[c + "/cat_tabel"])), c
        assert np.array_equal(bits(lst), bits(g[c + "/cat_list"])), c
        ref = np.zeros((C, 3))
        for t in batch_tables(g, c, False):
            ref = R.calc_categorical_iou(t, C, ref)
        assert np.array_equal(bits(calc), bits(ref)), c
    lp, tg = case(g, "s13", dev)
    hot = M.to_categorical(tg, 13)
    assert hot.is_cuda and hot.dtype == torch.float32 and hot.shape == (3, 1024, 13)
    assert torch.equal(hot.argmax(-1), tg) and float(hot.sum()) == 3 * 1024


def test_test_semseg_with_recorded_log_probs(dev):
    g = G()
    lps, tgs = batches_of(g, "s13")
    names = [str(n) for n in g["s3dis_names"]]
    catdict = dict(enumerate(names))
    loader = [(torch.zeros(lp.shape[0], lp.shape[1], 9), torch.from_numpy(tg)) for lp, tg in zip(lps, tgs)]
    acc, iou, cat_iou, _ = R.test_semseg(batch_tables(g, "s13", False), batch_points(g, "s13"), names, 13)
    for model_name, wrap in (("pointnet2", lambda lp: lp), ("pointnet", lambda lp: (lp, None))):
        stub = Stub(lps, dev, wrap)
        metrics, got = M.test_semseg(stub, iter(loader), catdict, model_name, 13)
        assert stub.args == [[(1, 9, 1024)]] * 3                                 # channel-first, as the reference feeds it
        assert bits(metrics["accuracy"]) == bits(acc) == bits(g["loop_semseg/accuracy"])
        assert bits(metrics["iou"]) == bits(iou) == bits(g["loop_semseg/iou"])
        assert list(got) == sorted(names) == [str(n) for n in g["loop_semseg/names"]]
        assert max(R.ulps(got[k], cat_iou[k]) for k in got) <= 4
        assert max(R.ulps(a, b) for a, b in zip(got.values(), g["loop_semseg/cat_iou"])) <= 4
    # grouped names: the mean of each group
    grouped = {i: "flat" if i < 3 else "thing" for i in range(13)}
    metrics, got = M.test_semseg(Stub(lps, dev), loader, grouped, "pointnet2", 13)
    _, _, want, tabel = R.test_semseg(batch_tables(g, "s13", False), batch_points(g, "s13"), [grouped[i] for i in range(13)], 13)
    assert list(got) == ["flat", "thing"] and max(R.ulps(got[k], want[k]) for k in got) <= 4
    assert R.ulps(got["thing"], np.mean(tabel[3:, 2])) <= 4


def test_test_partseg_with_recorded_log_probs(dev):
    g = G()
    lps, tgs = batches_of(g, "p50")
    names = [str(n) for n in g["part_names"]]
    catdict = dict(enumerate(names))
    loader = [(torch.zeros(2, 512, 3), torch.zeros(2, 1, dtype=torch.int64), torch.from_numpy(tg), torch.zeros(2, 512, 3)) for tg in tgs]
    want, hist, cat_iou = R.test_partseg(batch_tables(g, "p50", True), batch_points(g, "p50"), names, 50)
    for model_name, wrap, shapes in (("pointnet2", lambda lp: lp, [(2, 3, 512), (2, 3, 512), (2, 16)]),
                                     ("pointnet", lambda lp: (None, lp, None), [(2, 3, 512), (2, 16)])):
        stub = Stub(lps, dev, wrap)
        metrics, got_hist, got = M.test_partseg(stub, loader, catdict, model_name) if model_name == "pointnet2" else \
            M.test_partseg(stub, loader, catdict, model_name, 50)
        assert stub.args == [shapes] * 2
        assert bits(metrics["accuracy"]) == bits(want["accuracy"]) == bits(g["loop_partseg/accuracy"])
        assert bits(metrics["inctance_avg_iou"]) == bits(want["inctance_avg_iou"]) == bits(g["loop_partseg/inctance_avg_iou"])
        assert np.array_equal(bits(got_hist), bits(hist)) and np.array_equal(bits(got_hist), bits(g["loop_partseg/hist_acc"]))
        assert list(got) == list(cat_iou) == [str(n) for n in g["loop_partseg/names"]]
        assert max(R.ulps(got[k], cat_iou[k]) for k in got) <= 4
        assert max(R.ulps(a, b) for a, b in zip(got.values(), g["loop_partseg/cat_iou"])) <= 4
        assert R.ulps(metrics["class_avg_iou"], want["class_avg_iou"]) <= 4
        assert R.ulps(metrics["class_avg_iou"], g["loop_partseg/class_avg_iou"]) <= 4


def test_test_kitti_semseg_with_recorded_log_probs(dev, capsys):
    g = G()
    lps, tgs = batches_of(g, "k20")
    loader = [(torch.zeros(1, 2048, 4), torch.from_numpy(tg)) for tg in tgs]
    names = ["class%02d" % i for i in range(20)]
    acc, miou, per_class = R.test_kitti_semseg(batch_tables(g, "k20", False), batch_points(g, "k20"), 20)
    for model_name, wrap in (("pointnet2", lambda lp: lp), ("pointnet", lambda lp: (lp, None))):
        stub = Stub(lps, dev, wrap)
        got_acc, got_miou = M.test_kitti_semseg(stub, loader, model_name, 20, names)
        assert stub.args == [[(1, 4, 2048)]] * 2
        assert bits(got_acc) == bits(acc) and bits(got_miou) == bits(miou)
        text = capsys.readouterr().out
        assert "categorical mIOU" in text and all(n in text for n in names)
        best = names[int(np.argmax(per_class))]
        assert text.splitlines()[2].startswith(best)                             # sorted, best class first
    # class 0 starts at count 1 and is left out of the mean (pcdseg.py:61, :96)
    assert per_class[0] < 1 and bits(miou) == bits(np.mean(per_class[1:]))


def test_test_clf_with_recorded_log_probs(dev):
    g = G()
    lps, tgs = batches_of(g, "clf")
    loader = [(torch.zeros(8, 16, 3), torch.from_numpy(tg[0][:, None].copy())) for tg in tgs]
    stub = Stub([lp[0] for lp in lps], dev, lambda lp: (lp, None))
    got = M.test_clf(stub, loader)
    assert stub.args == [[(8, 3, 16)]] * 3
    assert bits(got) == bits(R.test_clf(batch_tables(g, "clf", False), [8, 8, 8])) == bits(g["loop_clf/accuracy"])


def test_test_semseg_end_to_end_on_a_real_network(dev):
    """Plumbing, not the network: the statistics of test_semseg on an eval-mode PointNet2SemSeg equal the same statistics computed
    from that model's own log-probabilities copied to the CPU."""
    from pointnet12_amd import pointnet2 as P
    from pointnet12_amd import synthetic as syn
    torch.manual_seed(3)
    net = P.PointNet2SemSeg(13, 6).to(dev).eval()
    seen = []

    def model(points):
        out = net(points)
        seen.append(out.detach().cpu())
        return out

    loader = []
    for i in range(2):
        pts, labels = syn.kitti_batch(2 * i, 2, 2048)
        labels[0, :50] = 13 + i                                                  # a few labels that are no class
        loader.append((torch.from_numpy(pts).transpose(2, 1), torch.from_numpy(labels)))
    names = ["n%02d" % (i // 2) for i in range(13)]
    metrics, cat_iou = M.test_semseg(model, loader, dict(enumerate(names)), "pointnet2", 13)
    assert len(seen) == 2 and seen[0].shape == (2, 2048, 13)
    tables = [R.count_tables(lp.argmax(-1).numpy(), tg.numpy(), 13).sum(0) for lp, (_, tg) in zip(seen, loader)]
    assert all(int(t[13].sum()) == 50 for t in tables)
    acc, iou, want, _ = R.test_semseg(tables, [2 * 2048] * 2, names, 13)
    assert bits(metrics["accuracy"]) == bits(acc) and bits(metrics["iou"]) == bits(iou)
    assert list(cat_iou) == list(want) and max(R.ulps(cat_iou[k], want[k]) for k in want) <= 4
