"""GPU: pn2_seg_confusion at the C ABI (ctypes) on the launch plans tests/test_metrics_gpu.py never reaches at 256 compute units:
the row loop's second and partly-live last trip, the 2-copy LDS table of C = 64 (and the 64 512-byte one of C = 63), the 16th quad
of the row arg-max, and the wave combine at exactly 1, 4, 5 and 64 distinct bins.

A cloud gets wgs = max(min(cdiv(N, 256), cdiv(8 * CUs, B)), cdiv(N, 2^31)) workgroups, each walking strides of wgs * 256 rows
(``plan`` restates it; every case asserts the trips it was built for and prints its plan).  Everything is integers and must be
EQUAL: the tables to torch.bincount over (label row, prediction) of the CPU copies, the predictions to an arg-max spelt out in
numpy (lowest index of the maximum; the first NaN wins).  conf and pred sit between guard words that must come back unchanged."""
import numpy as np
import pytest
import torch

from pointnet12_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
CONF_SENT, PRED_SENT = -777, -555
NAN, INF = float("nan"), float("inf")


def cdiv(a, b):
    return -(-a // b)


def plan(B, N, C, cus):
    """-> workgroups per cloud, trips of each workgroup, live rows in the last trip of each workgroup, table copies in LDS."""
    wgs = max(min(cdiv(N, 256), cdiv(8 * cus, B)), cdiv(N, 1 << 31))
    stride = wgs * 256
    trips = [cdiv(N - w * 256, stride) for w in range(wgs)]
    last = [min(256, N - w * 256 - (t - 1) * stride) for w, t in zip(range(wgs), trips)]
    return wgs, trips, last, 4 if 4 * (C + 1) * C * 4 <= 64 * 1024 else 2


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def argmax_rows(x):
    """numpy [R, C] -> the contract's prediction: the lowest index of the largest entry; a NaN is largest and the first one wins."""
    isnan = np.isnan(x)
    plain = np.where(isnan, -np.inf, x)
    first_max = (plain == plain.max(axis=1, keepdims=True)).argmax(axis=1)
    return np.where(isnan.any(axis=1), isnan.argmax(axis=1), first_max).astype(np.int64)


def tables(pred, target, B, C, per_cloud, ignore=None):
    """torch.bincount over (cloud, label row, prediction) of CPU tensors; rows whose label is `ignore` are left out."""
    N = target.shape[1]
    row = torch.where((target >= 0) & (target < C), target, torch.full_like(target, C))
    cloud = torch.arange(B)[:, None].expand(B, N) if per_cloud else torch.zeros(B, N, dtype=torch.int64)
    flat = ((cloud * (C + 1) + row) * C + pred).reshape(-1)
    if ignore is not None:
        flat = flat[target.reshape(-1) != ignore]
    nb = B if per_cloud else 1
    return torch.bincount(flat, minlength=nb * (C + 1) * C).view(nb, C + 1, C)


def rows_on_device(lp, ld, shift, dev, fill=(NAN, INF)):
    """lp [B, N, C] (CPU) as rows of pitch ld in a device buffer whose pad columns hold `fill` alternating; shift = 1 starts the rows
    one float off a 16-byte boundary.  -> (the buffer, kept alive by the caller; the pointer of row 0)."""
    B, N, C = lp.shape
    store = torch.empty(B * N * ld + shift + 3, device=dev, dtype=torch.float32)
    store.fill_(fill[0])
    buf = store[shift:shift + B * N * ld].view(B * N, ld)
    buf[:, 0::2] = fill[0]
    buf[:, 1::2] = fill[1]
    buf[:, :C] = lp.reshape(B * N, C).to(dev)
    assert store.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 4 * shift
    return store, buf.data_ptr()


def launch(dev, lp, target, ld=None, shift=0, per_cloud=True, ignore=None, want_pred=True, fill=(NAN, INF), pred_ref=None, what=""):
    """One framed call; asserts the return code, the guards, the table and the predictions."""
    lib = _lib.load()
    B, N, C = lp.shape
    ld = C if ld is None else ld
    store, ptr = rows_on_device(lp, ld, shift, dev, fill)
    nb = B if per_cloud else 1
    size = nb * (C + 1) * C
    conf = torch.full((size + 2 * GUARD,), CONF_SENT, dtype=torch.int64, device=dev)
    conf[GUARD:GUARD + size] = 0
    pred = torch.full((B * N + 2 * GUARD,), PRED_SENT, dtype=torch.int64, device=dev)
    t = target.to(dev)
    ignore_value = -(1 << 62) if ignore is None else ignore                   # no label holds it
    assert ignore is not None or not bool((target == ignore_value).any())
    rc = lib.pn2_seg_confusion(ptr, ld, t.data_ptr(), B, N, C, ignore_value, conf[GUARD:].data_ptr(), (C + 1) * C if per_cloud else 0,
                               pred[GUARD:].data_ptr() if want_pred else None, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    conf, pred = conf.cpu(), pred.cpu()
    assert bool((conf[:GUARD] == CONF_SENT).all()) and bool((conf[GUARD + size:] == CONF_SENT).all()), "%s: a guard of conf was written" % what
    assert bool((pred[:GUARD] == PRED_SENT).all()) and bool((pred[GUARD + B * N:] == PRED_SENT).all()), "%s: a guard of pred was written" % what
    if pred_ref is None:
        pred_ref = torch.from_numpy(argmax_rows(lp.reshape(B * N, C).numpy())).view(B, N)
    if want_pred:
        assert torch.equal(pred[GUARD:GUARD + B * N].view(B, N), pred_ref), "%s: predictions differ" % what
    else:
        assert bool((pred == PRED_SENT).all()), "%s: pred = NULL was written" % what
    want = tables(pred_ref, target, B, C, per_cloud, ignore)
    got = conf[GUARD:GUARD + size].view(nb, C + 1, C)
    assert torch.equal(got, want), "%s: %d table entries differ" % (what, int((got != want).sum()))
    return got, pred_ref


def drawn(seed, B, N, C, strays=True, runs=16):
    """CPU log-probabilities that favour the label, labels in runs of `runs`, a few labels that are no class (-1, C, 255)."""
    gen = torch.Generator().manual_seed(seed)
    target = torch.randint(0, C, (B, cdiv(N, runs)), generator=gen).repeat_interleave(runs, dim=1)[:, :N].contiguous()
    logits = torch.randn(B, N, C, generator=gen)
    logits.scatter_add_(2, target[:, :, None], torch.full((B, N, 1), 1.5))
    lp = torch.log_softmax(logits, -1)
    if strays:
        where = torch.randint(0, N, (B, 48), generator=gen)
        target.scatter_(1, where, torch.tensor([-1, C, 255]).repeat(B, 16))
    return lp, target


def announce(dev, name, B, N, C):
    wgs, trips, last, copies = plan(B, N, C, cus_of(dev))
    print("confusion %-28s B %d N %d C %d  CUs %d  workgroups/cloud %d  trips %s  live rows in the last trip %s  LDS copies %d (%d bytes)"
          % (name, B, N, C, cus_of(dev), wgs, sorted(set(trips)), sorted(set(last)), copies, copies * (C + 1) * C * 4))
    return wgs, trips, last, copies


@pytest.mark.parametrize("ld", [3, 4], ids=["scalar-rows", "quad-rows"])
def test_one_workgroup_per_cloud_four_trips_ragged_last(dev, ld):
    B, N, C = 4096, 3 * 256 + 37, 3
    wgs, trips, last, _ = announce(dev, "four trips, 37 live", B, N, C)
    assert wgs == 1 and trips == [4] and last == [37]               # cdiv(8 * CUs, 4096) == 1 up to 512 compute units
    lp, target = drawn(1, B, N, C, runs=5)
    _, pred_ref = launch(dev, lp, target, ld=ld, per_cloud=True, what="per cloud")
    pooled, _ = launch(dev, lp, target, ld=ld, per_cloud=False, pred_ref=pred_ref, what="pooled")
    assert int(pooled.sum()) == B * N and int(pooled[0, C].sum()) > 0


def test_kitti_like_batch_two_trips_19_live_rows(dev):
    cus = cus_of(dev)
    B, C = 16, 13
    N = 256 * cdiv(8 * cus, 16) + 275
    wgs, trips, last, _ = announce(dev, "KITTI-like batch", B, N, C)
    assert wgs == cdiv(8 * cus, 16) and trips[:3] == [2, 2, 1][:wgs] and last[:2] == [256, 19] and set(trips[2:]) <= {1}
    lp, target = drawn(2, B, N, C)
    label = int(target[0, 0])
    _, pred_ref = launch(dev, lp, target, what="no ignore_index")
    for ignore in (label, 255, -1):
        assert bool((target == ignore).any())
        for want_pred in (True, False):
            for per_cloud in (True, False):
                launch(dev, lp, target, ignore=ignore, want_pred=want_pred, per_cloud=per_cloud, pred_ref=pred_ref,
                       what="ignore %d, pred %s, per cloud %s" % (ignore, want_pred, per_cloud))
    launch(dev, lp, target, want_pred=False, per_cloud=False, pred_ref=pred_ref, what="pooled, pred = NULL")
    launch(dev, lp, target, ld=16, pred_ref=pred_ref, what="ld 16")


def plant_rows(lp, C):
    """Rows whose maximum, a tie and a first NaN sit in the last columns (60 .. 63 where there are that many)."""
    lo = max(0, C - 4)
    r = 0
    for c in range(lo, C):
        lp[0, r] = -3.0
        lp[0, r, c] = 0.5                                           # the maximum alone in column c
        r += 1
        lp[0, r] = -3.0
        lp[0, r, c:] = 0.5                                          # a tie from c to the end: c wins
        r += 1
        lp[0, r] = -3.0
        lp[0, r, c:] = NAN                                          # NaNs from c to the end: the first wins
        lp[0, r, 0] = 9.0
        r += 1
        lp[0, r] = -INF
        lp[0, r, c] = -1e30                                         # everything else -inf
        r += 1
    lp[0, r] = -INF                                                 # all -inf: 0
    lp[0, r + 1] = INF                                              # all +inf: 0
    lp[0, r + 2] = NAN                                              # all NaN: 0
    want = [v for c in range(lo, C) for v in (c, c, c, c)] + [0, 0, 0]
    return r + 3, want


@pytest.mark.parametrize("C", [1, 61, 62, 63, 64])
def test_class_counts_around_the_two_copy_table(dev, C):
    B, N = 2, 1000
    _, _, _, copies = announce(dev, "C = %d" % C, B, N, C)
    assert copies == (2 if C == 64 else 4)
    lp, target = drawn(30 + C, B, N, C)
    gen = torch.Generator().manual_seed(C)
    target[1] = torch.randint(0, C, (N,), generator=gen)                      # cloud 1: labels over all classes, no runs
    lp[1] = torch.log_softmax(torch.randn(N, C, generator=gen), -1)           # ... and predictions over all classes
    target[1, ::97] = torch.tensor([-1, C, 255]).repeat(4)[:len(target[1, ::97])]
    rows, want = plant_rows(lp, C)
    pred_ref = torch.from_numpy(argmax_rows(lp.reshape(B * N, C).numpy())).view(B, N)
    assert pred_ref[0, :rows].tolist() == want
    assert len(set(pred_ref[1].tolist())) == C and len(set(target[1].tolist())) >= min(C, 60)
    layouts = [((C + 3) & ~3, 0, "round4(C), aligned: quads"), (C + 1, 1, "C + 1 from a base one float off 16 bytes: scalar")]
    if C % 4 == 0:                                                              # (round4(C) == C: no pad above; here with one)
        layouts.append((C + 4, 0, "C + 4, aligned: quads with a pad quad"))
    for ld, shift, what in layouts:
        for fill in ((NAN, INF), (INF, NAN)):                                   # at C = 63, ld = 64: column 63 holds NaN or +inf
            for per_cloud in (True, False):
                launch(dev, lp, target, ld=ld, shift=shift, fill=fill, per_cloud=per_cloud, pred_ref=pred_ref, what="C %d, %s" % (C, what))
    launch(dev, lp, target, ld=(C + 3) & ~3, ignore=255, pred_ref=pred_ref, what="C %d, ignore 255" % C)


def test_wave_combine_at_1_4_5_and_64_bins(dev):
    """One workgroup (four waves of 64 rows) per 256 rows: waves with exactly 1, 4, 5 and 64 distinct (label, prediction) bins -- up
    to four keys are counted by ballot, the rest lane by lane -- and a wave whose odd lanes are ignored rows."""
    B, N, C, ignore = 1, 512, 13, 99
    wgs, trips, _, _ = announce(dev, "wave combine", B, N, C)
    assert wgs == 2 and trips == [1, 1]
    gen = torch.Generator().manual_seed(4)
    target = torch.randint(0, C, (B, N), generator=gen)
    pred = torch.randint(0, C, (B, N), generator=gen)
    lane = torch.arange(64)
    plant = {0: (lane * 0 + 3, lane * 0 + 7),                                   # one bin
             1: (lane % 4, lane * 0 + 2),                                       # four bins
             2: (lane % 5, (lane % 5 + 1) % C),                                 # five bins: one is left to the single lanes
             3: (torch.where(lane < 52, lane // 4, torch.full_like(lane, 200)), torch.where(lane < 52, lane % 4, lane - 52)),   # 64 bins
             5: (torch.where(lane % 2 == 1, torch.full_like(lane, ignore), lane // 2 % 3), lane // 2 % 2)}    # odd lanes ignored
    for w, (t, p) in plant.items():
        target[0, 64 * w:64 * w + 64] = t
        pred[0, 64 * w:64 * w + 64] = p
    lp = torch.full((B, N, C), -5.0)
    lp.scatter_(2, pred[:, :, None], 0.0)

    def distinct(w, live=None):
        t, p = target[0, 64 * w:64 * w + 64], pred[0, 64 * w:64 * w + 64]
        row = torch.where((t >= 0) & (t < C), t, torch.full_like(t, C))
        keys = row * C + p
        return len(set((keys if live is None else keys[live]).tolist()))

    assert [distinct(w) for w in (0, 1, 2, 3)] == [1, 4, 5, 64]
    assert distinct(5, target[0, 320:384] != ignore) == 6 and int((target[0, 320:384] == ignore).sum()) == 32
    got, _ = launch(dev, lp, target, ignore=ignore, pred_ref=pred, what="wave combine")
    assert int(got.sum()) == N - 32 - int((target[0] == ignore).sum() - 32)
    launch(dev, lp, target, pred_ref=pred, what="wave combine, nothing ignored")
    launch(dev, lp, target, ld=16, per_cloud=False, ignore=ignore, pred_ref=pred, what="wave combine, quads, pooled")


def test_65_classes_are_still_refused(dev):
    lib = _lib.load()
    B, N, C = 2, 300, 65
    lp = torch.zeros(B, N, C, device=dev)
    target = torch.zeros(B, N, dtype=torch.int64, device=dev)
    conf = torch.full((B * (C + 1) * C + 2 * GUARD,), CONF_SENT, dtype=torch.int64, device=dev)
    pred = torch.full((B * N + 2 * GUARD,), PRED_SENT, dtype=torch.int64, device=dev)
    rc = lib.pn2_seg_confusion(lp.data_ptr(), C, target.data_ptr(), B, N, C, -100, conf[GUARD:].data_ptr(), (C + 1) * C,
                               pred[GUARD:].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc == _lib.PN2_EUNSUPPORTED
    assert bool((conf == CONF_SENT).all()) and bool((pred == PRED_SENT).all())
