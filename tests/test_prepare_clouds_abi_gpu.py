"""GPU: pn2_prepare_clouds at the C ABI on the paths pointnet12_amd/loader.py never takes (it passes bad_index = NULL and valid draws):
an out-of-range ``choice`` (flagged, row 0 used), a cloud with ``row_count`` 0 (zeros, label 0), the optional pointers, and the
refusals.  Expected values are ``oracle/train_ref.normalize`` and numpy indexing; every comparison is on raw fp32 bits (a NaN
coordinate included: it passes the clip as through np.clip), and points and labels sit between guard rows."""
import numpy as np
import pytest
import torch

from oracle import train_ref as TR
from pointnet12_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL = -1
M0, M2 = 37, 301                            # rows of the two real clouds; an empty one lies between them
P_SENT, L_SENT = 7.5, -77                   # what points and labels hold before a call
_p = _lib.ptr


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scans():
    """raw [M0 + M2, 4], labels, and a noise table laid out differently (a distinct constant per cloud plus a per-row ramp)."""
    rng = np.random.default_rng(12)
    M = M0 + M2
    raw = np.concatenate([rng.uniform(-90, 90, (M, 2)), rng.uniform(-4, 4, (M, 1)), rng.uniform(-0.2, 1.2, (M, 1))], 1).astype(np.float32)
    nxt = np.nextafter(np.float32(70), np.float32(100))
    raw[0] = (70, -70, 3, 0.5)                                      # exactly on the clip: +-1
    raw[1] = (-70, 70, -3, 1.0)
    raw[2] = (-0.0, 0.0, -0.0, 0.0)
    raw[3] = (np.nan, 1.0, 1.0, 0.3)                                # passes through
    raw[4] = (nxt, -1e30, np.inf, -np.inf)                          # beyond: clipped
    raw[5] = (-nxt, 1e30, -np.inf, 7.0)
    raw[M0] = (-0.0, 71.0, -3.0, 1.5)                               # row 0 of the second real cloud
    label = rng.integers(1, 20, M).astype(np.int32)                 # never 0: a label 0 is one that was written as such
    nb = np.array([5, 0, 5 + M0 + 3], np.int64)                     # != row_begin for every cloud
    noise = np.full((nb[2] + M2 + 2, 4), 9.0, np.float32)
    for b, (lo, cnt) in enumerate(((nb[0], M0), (0, 0), (nb[2], M2))):
        ramp = (0.01 * (b + 1) + 1e-5 * np.arange(cnt))[:, None] * np.array([1, -1, 0.5, 2.0])
        noise[lo:lo + cnt] = ramp.astype(np.float32)
    return raw, label, noise, nb


def draws(N, rng, counts):
    """[B, N] valid draws; each real cloud's begin with its first rows, so that the planted rows are read."""
    out = np.zeros((len(counts), N), np.int64)
    for b, M in enumerate(counts):
        if M > 0:
            out[b] = np.concatenate([np.arange(M), rng.integers(0, M, N)])[:N]
    return out


def expected(raw, label, begin, count, choice, noise=None, noise_begin=None):
    B, N = choice.shape
    pts, lab, bad = np.zeros((B, N, 4), np.float32), np.zeros((B, N), np.int64), 0
    for b in range(B):
        lo, M = int(begin[b]), int(count[b])
        c = choice[b].copy()
        oob = (c < 0) | (c >= M)
        bad |= int(oob.any())
        if M <= 0:
            continue                                                # zeros, label 0
        c[oob] = 0
        with np.errstate(invalid="ignore"):
            rows = TR.normalize(raw[lo:lo + M])
            if noise is not None:
                nlo = int(noise_begin[b]) if noise_begin is not None else lo
                rows = noise[nlo:nlo + M] + rows
        pts[b] = rows[c]
        if label is not None:
            lab[b] = label[lo:lo + M][c]
    return pts, lab, bad


class Call:
    """Device copies of one call's operands; points and labels guarded by a row in front and one behind."""

    def __init__(self, dev, raw, label, begin, count, choice, noise=None, noise_begin=None):
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.B, self.N = choice.shape
        self.raw, self.label, self.begin, self.count = t(raw), t(label), t(begin), t(count)
        self.choice, self.noise, self.noise_begin = t(choice.reshape(-1)), t(noise), t(noise_begin)
        rows = self.B * self.N
        self.p_hold = torch.full((rows + 2, 4), P_SENT, device=dev)
        self.l_hold = torch.full((rows + 2,), L_SENT, dtype=torch.int64, device=dev)
        self.points, self.labels = self.p_hold[1:-1], self.l_hold[1:-1]
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        assert self.points.data_ptr() % 16 == 0 and self.raw.data_ptr() % 16 == 0

    def run(self, labels=True, bad=True, **swap):
        a = dict(raw=_p(self.raw), begin=_p(self.begin), count=_p(self.count), label=_p(self.label), noise=_p(self.noise),
                 noise_begin=_p(self.noise_begin), choice=_p(self.choice), B=self.B, N=self.N, points=_p(self.points),
                 labels=_p(self.labels) if labels else None, bad=_p(self.bad) if bad else None)
        a.update(swap)
        rc = _lib.load().pn2_prepare_clouds(a["raw"], a["begin"], a["count"], a["label"], a["noise"], a["noise_begin"], a["choice"],
                                            a["B"], a["N"], a["points"], a["labels"], a["bad"], _lib.stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        p, l = self.p_hold.cpu().numpy(), self.l_hold.cpu().numpy()
        assert (p[[0, -1]] == P_SENT).all() and (l[[0, -1]] == L_SENT).all(), "a guard row was written"
        return p[1:-1].reshape(self.B, self.N, 4), l[1:-1].reshape(self.B, self.N), int(self.bad.item())

    def untouched(self):
        return bool((self.p_hold == P_SENT).all()) and bool((self.l_hold == L_SENT).all())


def same(call, want, what, labels=True):
    pts, lab, bad = call.outputs()
    differ = bits(pts) != bits(want[0])
    assert not differ.any(), "%s: %d point values differ, first at %s" % (what, int(differ.sum()), np.argwhere(differ)[0])
    if labels:
        assert (lab == want[1]).all(), what
    assert bad == want[2], what


BEGIN = np.array([0, M0, M0], np.int64)
COUNT = np.array([M0, 0, M2], np.int64)
COUNT_FULL = np.array([M0, M0, M2], np.int64)                      # "no empty cloud": the middle one is the first again
BEGIN_FULL = np.array([0, 0, M0], np.int64)


# ------------------------------------------------------------------------------------------------ 1. reference, empty cloud
@pytest.mark.parametrize("jitter", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("N", [1, 64, 255, 257])
def test_prepare_clouds_reference_and_empty_cloud(dev, N, jitter):
    """B = 3 (B N no multiple of the 256-thread workgroup for N = 1, 255, 257): two real clouds around one with row_count = 0,
    whose rows are zeros with label 0 and which raises the flag; without it, with valid draws, the flag stays 0."""
    raw, label, noise, nb = scans()
    rng = np.random.default_rng(N)
    noise, nb = (noise, nb) if jitter else (None, None)
    choice = draws(N, rng, COUNT)
    choice[1] = rng.integers(-3, 40, N)                             # whatever is drawn for the empty cloud
    call = Call(dev, raw, label, BEGIN, COUNT, choice, noise, nb)
    assert call.run() == 0
    want = expected(raw, label, BEGIN, COUNT, choice, noise, nb)
    assert want[2] == 1 and not want[0][1].any() and not want[1][1].any() and want[1][0].all()
    same(call, want, "empty cloud in the middle")
    # no empty cloud, valid draws: the flag is not raised
    choice = draws(N, rng, COUNT_FULL)
    nb_full = None if nb is None else np.array([nb[0], nb[0], nb[2]], np.int64)
    call = Call(dev, raw, label, BEGIN_FULL, COUNT_FULL, choice, noise, nb_full)
    assert call.run() == 0
    want = expected(raw, label, BEGIN_FULL, COUNT_FULL, choice, noise, nb_full)
    assert want[2] == 0
    same(call, want, "no empty cloud")
    if N >= 6:                                                      # the planted rows were read: +-1, -0, NaN
        w = bits(want[0][0, :6] if not jitter else TR.normalize(raw[:6]))
        assert w[0].tolist() == bits(np.array([1, -1, 1, 0], np.float32)).tolist() and w[2, 0] == 0x80000000
        assert w[3, 0] == 0x7fc00000 and w[4].tolist() == bits(np.array([1, -1, 1, -1], np.float32)).tolist()


# ------------------------------------------------------------------------------------------------ 2. bad draws
@pytest.mark.parametrize("jitter", [False, True], ids=["plain", "noise"])
def test_prepare_clouds_out_of_range_choice(dev, jitter):
    """One draw of -1 and one of row_count (one past the end): flagged, and those two rows are row 0 of their cloud -- with noise, row 0
    plus row 0's noise -- with row 0's label.  bad_index = NULL: the same bytes, nothing flagged, still accepted."""
    raw, label, noise, nb = scans()
    noise, nb = (noise, nb) if jitter else (None, None)
    N = 64
    choice = draws(N, np.random.default_rng(3), COUNT)
    choice[0, 9], choice[2, 40] = -1, M2
    call = Call(dev, raw, label, BEGIN, COUNT, choice, noise, nb)
    assert call.run() == 0
    want = expected(raw, label, BEGIN, COUNT, choice, noise, nb)
    same(call, want, "bad draws")
    pts, lab, bad = call.outputs()
    assert bad == 1
    for b, n, lo, nlo in ((0, 9, 0, 5), (2, 40, M0, 5 + M0 + 3)):
        row0 = TR.normalize(raw[lo:lo + 1])[0]
        if jitter:
            row0 = noise[nlo] + row0
        assert (bits(pts[b, n]) == bits(row0)).all() and lab[b, n] == label[lo]
    # the same bad draws in real clouds only: the flag comes from them alone
    choice_full = choice.copy()
    choice_full[1] = np.arange(N) % M0
    nb_full = None if nb is None else np.array([nb[0], nb[0], nb[2]], np.int64)
    call = Call(dev, raw, label, BEGIN_FULL, COUNT_FULL, choice_full, noise, nb_full)
    assert call.run() == 0
    same(call, expected(raw, label, BEGIN_FULL, COUNT_FULL, choice_full, noise, nb_full), "bad draws, no empty cloud")
    assert call.outputs()[2] == 1
    # bad_index = NULL
    blind = Call(dev, raw, label, BEGIN, COUNT, choice, noise, nb)
    assert blind.run(bad=False) == 0
    same(blind, want[:2] + (0,), "bad_index = NULL")


# ------------------------------------------------------------------------------------------------ 3. optional pointers
def test_prepare_clouds_optional_pointers(dev):
    raw, label, noise, nb = scans()
    N = 255
    choice = draws(N, np.random.default_rng(4), COUNT)
    want = expected(raw, label, BEGIN, COUNT, choice)
    # labels = NULL: points as ever, nothing written for labels
    call = Call(dev, raw, label, BEGIN, COUNT, choice)
    assert call.run(labels=False) == 0
    same(call, want, "labels = NULL", labels=False)
    assert bool((call.l_hold == L_SENT).all())
    # raw_label = NULL with labels given: every label 0
    call = Call(dev, raw, None, BEGIN, COUNT, choice)
    assert call.run() == 0
    same(call, expected(raw, None, BEGIN, COUNT, choice), "raw_label = NULL")
    assert not call.outputs()[1].any()
    # noise with a noise_begin of its own: each cloud's noise is read from its own offset ...
    assert (nb != BEGIN).all()
    call = Call(dev, raw, label, BEGIN, COUNT, choice, noise, nb)
    assert call.run() == 0
    with_own = expected(raw, label, BEGIN, COUNT, choice, noise, nb)
    same(call, with_own, "noise_begin given")
    # ... and with noise_begin = NULL at row_begin, which is other rows of the table
    call = Call(dev, raw, label, BEGIN, COUNT, choice, noise, None)
    assert call.run() == 0
    at_rows = expected(raw, label, BEGIN, COUNT, choice, noise, None)
    same(call, at_rows, "noise_begin = NULL")
    assert (bits(at_rows[0]) != bits(with_own[0])).any() and (bits(with_own[0]) != bits(want[0])).any()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_prepare_clouds_refusals_launch_nothing(dev):
    """Each case fails a host-side PN2_CHECK_ARG of pn2_prepare_clouds before any launch: -1, points and labels keep their sentinels."""
    raw, label, noise, nb = scans()
    N = 16
    choice = draws(N, np.random.default_rng(5), COUNT)
    call = Call(dev, raw, label, BEGIN, COUNT, choice, noise, nb)
    off = lambda t: t.reshape(-1)[1:].data_ptr()                    # 4 bytes off a 16-byte boundary
    assert off(call.raw) % 16 == 4 and off(call.p_hold) % 16 == 4 and off(call.noise) % 16 == 4
    cases = [dict(raw=off(call.raw)), dict(points=off(call.p_hold)), dict(noise=off(call.noise)),
             dict(raw=None), dict(begin=None), dict(count=None), dict(choice=None), dict(points=None), dict(B=0), dict(N=0),
             dict(B=-1), dict(N=-1)]
    for kw in cases:
        assert call.run(**kw) == EINVAL, kw
        assert call.untouched(), kw
    assert int(call.bad.item()) == 0
    assert call.run() == 0 and not call.untouched()                 # the same operands, un-swapped, are accepted
