"""GPU: pn2_sample_image and pn2_hsv_to_rgb at the C ABI against the numpy statements of tests/image_sample_ref.py, bit for bit."""
import numpy as np
import pytest
import torch

import image_sample_ref as R
from pointnet12_amd import _lib

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SENTINEL = 0x7fc0dead                     # a quiet NaN with a payload, as int32 bits
VALID_SENTINEL = 0xab
FORMS = [("rgb", 0), ("rgb", 1), ("hsv", 0), ("hsv", 1)]
MODE = {"rgb": _lib.IMAGE_RGB, "hsv": _lib.IMAGE_HSV}
ORDER = {"rgb": _lib.CHANNELS_RGB, "bgr": _lib.CHANNELS_BGR}
p = _lib.ptr


def sample(pix, image, B, H, W, order, mode, norm, begin, count, max_rows, out, ldo, valid, rows=None, err=None):
    """``rows`` (how many rows the buffers hold) defaults to the rows of ``pix``."""
    return _lib.load().pn2_sample_image(p(pix), p(image), B, H, W, ORDER[order], MODE[mode], norm, p(begin), p(count), max_rows,
                                        pix.shape[0] if rows is None else rows, p(out), ldo, p(valid), p(err), _lib.stream())


def bits(t):
    return t.contiguous().view(torch.int32)


def sentinel_rows(rows, ld, dev):
    return torch.full((rows, ld), SENTINEL, device=dev, dtype=torch.int32).view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------- all colours
@pytest.fixture(scope="module")
def all_colours(dev):
    """Every colour once: a 4096 x 4096 image whose pixel number c (row-major) holds the bytes (c >> 16, c >> 8 & 255, c & 255), the
    identity pixels, and the numpy statement's colours in the four forms (computed once)."""
    c = np.arange(1 << 24, dtype=np.int64)
    chan = [(c >> 16) & 255, (c >> 8) & 255, c & 255]
    image = torch.from_numpy(np.stack(chan, -1).astype(np.uint8).reshape(4096, 4096, 3)).to(dev)
    pix = torch.from_numpy(np.stack([c & 4095, c >> 12], -1).astype(np.int32)).to(dev)
    want = {}
    for order in ("rgb", "bgr"):
        r, g, b = chan if order == "rgb" else chan[::-1]
        for mode, planes in (("rgb", (r, g, b)), ("hsv", R.hsv_u8(r, g, b))):
            raw = np.stack(planes, -1).astype(np.float32)
            want[order, mode, 0] = torch.from_numpy(raw).to(dev)
            want[order, mode, 1] = torch.from_numpy(R.normalize_colors(raw, mode)).to(dev)     # (in place: numpy's float32 `/=`)
    return image, pix, want


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_all_colours_in_the_four_forms(dev, all_colours, order):
    image, pix, want = all_colours
    n = 1 << 24
    out = torch.empty(n, 3, device=dev, dtype=torch.float32)
    valid = torch.empty(n, device=dev, dtype=torch.uint8)
    for mode, norm in FORMS:                                          # every expectation is the numpy statement's own array
        out.fill_(-1.0)
        assert sample(pix, image, 1, 4096, 4096, order, mode, norm, None, None, n, out, 3, valid) == 0
        assert torch.equal(bits(out), bits(want[order, mode, norm])), (order, mode, norm)
        assert bool((valid == 1).all())


# -------------------------------------------------------------------------------------------- coordinates, sizes, rows, pitches
def edge_points(H, W, n, seed):
    """Every pair of the coordinates -2^31, -1, 0, W - 1, W, H - 1, H, 2^31 - 1 (each in either component, and in both), then
    random points in and around the image up to ``n`` rows."""
    vals = sorted({INT32_MIN, -1, 0, W - 1, W, H - 1, H, INT32_MAX})
    pts = [(x, y) for x in vals for y in vals]
    rng = np.random.RandomState(seed)
    while len(pts) < n:
        pts.append((int(rng.randint(-2, W + 2)), int(rng.randint(-2, H + 2))))
    pts = np.array(pts, np.int64)
    return pts[rng.permutation(len(pts))].astype(np.int32)


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (375, 1242)])
def test_coordinates_rows_pitches_and_valid(dev, size):
    H, W = size
    rng = np.random.RandomState(H * 7 + W)
    image_np = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    image = torch.from_numpy(image_np).to(dev)
    guard, case = 3, 0
    all_pts = edge_points(H, W, 257, H + W)                           # shuffled: every N holds a mix, N = 257 holds every pair
    for N in (1, 63, 64, 65, 257):
        pts_np = np.ascontiguousarray(all_pts[:N])
        pix = torch.from_numpy(pts_np).to(dev)
        for ldo in (3, 4, 7, 8):
            for with_valid in (True, False):
                mode, norm = FORMS[case % 4]
                order = ("rgb", "bgr")[(case // 4) % 2]
                case += 1
                col0 = ldo - 3                                       # the three columns are the LAST of the row: a pointer into it
                buf = sentinel_rows(N + guard, ldo, dev)
                valid = torch.full((N + guard,), VALID_SENTINEL, device=dev, dtype=torch.uint8)
                rc = sample(pix, image, 1, H, W, order, mode, norm, None, None, N, buf[:, col0:], ldo, valid if with_valid else None)
                assert rc == 0
                exp, exp_valid = R.sample_image(pts_np, image_np, mode, bool(norm), order)
                got = buf.cpu().numpy()
                assert got[:N, col0:].tobytes() == exp.tobytes(), (size, N, ldo, mode, norm, order)
                raw = got.view(np.int32)
                assert (raw[:N, :col0] == SENTINEL).all() and (raw[N:] == SENTINEL).all()
                v = valid.cpu().numpy()
                if with_valid:
                    assert (v[:N] == exp_valid).all() and (v[N:] == VALID_SENTINEL).all()
                else:
                    assert (v == VALID_SENTINEL).all()
                assert not np.signbit(exp[~exp_valid]).any() and (exp[~exp_valid] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------- batched
def batch_setup(dev, max_rows=70, H=6, W=9):
    rng = np.random.RandomState(3)
    base = rng.randint(0, 256, (H, W, 3)).astype(np.int64)
    images_np = np.stack([(base + 85 * b) % 256 for b in range(3)]).astype(np.uint8)     # the images differ in every pixel
    assert all((images_np[a] != images_np[b]).all() for a in range(3) for b in range(a))
    begins = np.array([2, 2 + max_rows + 4, 2 + 2 * (max_rows + 4)], np.int64)          # gaps between the clouds and at both ends
    rows = int(begins[-1]) + max_rows + 5
    pts_np = np.stack([rng.randint(-2, W + 2, rows), rng.randint(-2, H + 2, rows)], -1).astype(np.int32)
    return images_np, begins, rows, pts_np


def batch_expected(images_np, begins, counts, max_rows, pts_np, rows, mode, norm, order, onto=None):
    """What the buffers hold after a call: the sentinel (or ``onto``, what an earlier call left) outside the counted rows."""
    exp = np.full((rows, 3), SENTINEL, np.int32) if onto is None else onto[0].copy()
    exp_valid = np.full(rows, VALID_SENTINEL, np.uint8) if onto is None else onto[1].copy()
    for b in range(3):
        n = min(max(int(counts[b]), 0), max_rows)
        lo = int(begins[b])
        c, v = R.sample_image(pts_np[lo:lo + n], images_np[b], mode, bool(norm), order)
        exp[lo:lo + n] = c.view(np.int32)
        exp_valid[lo:lo + n] = v
    return exp, exp_valid


def test_batched_counts_and_each_cloud_reads_its_own_image(dev):
    max_rows = 70
    images_np, begins, rows, pts_np = batch_setup(dev, max_rows)
    image, pix = torch.from_numpy(images_np).to(dev), torch.from_numpy(pts_np).to(dev)
    begin = torch.from_numpy(begins).to(dev)
    count = torch.zeros(3, device=dev, dtype=torch.int64)
    for k, (mode, norm) in enumerate(FORMS):
        order = ("rgb", "bgr")[k % 2]
        out = sentinel_rows(rows, 3, dev)
        valid = torch.full((rows,), VALID_SENTINEL, device=dev, dtype=torch.uint8)
        held = None
        for counts in ((max_rows, 0, -1), (5, max_rows, 1)):            # the second call on the SAME buffers, as the first left them
            count.copy_(torch.tensor(counts))
            assert sample(pix, image, 3, 6, 9, order, mode, norm, begin, count, max_rows, out, 3, valid) == 0
            held = exp, exp_valid = batch_expected(images_np, begins, counts, max_rows, pts_np, rows, mode, norm, order, held)
            assert (out.cpu().numpy().view(np.int32) == exp).all(), (mode, norm, counts)
            assert (valid.cpu().numpy() == exp_valid).all()
    # a count above max_rows is clamped to it
    count.copy_(torch.tensor((max_rows + 3, 2, 0)))
    out.view(torch.int32).fill_(SENTINEL)
    assert sample(pix, image, 3, 6, 9, "rgb", "rgb", 0, begin, count, max_rows, out, 3, None) == 0
    exp, _ = batch_expected(images_np, begins, (max_rows, 2, 0), max_rows, pts_np, rows, "rgb", 0, "rgb")
    assert (out.cpu().numpy().view(np.int32) == exp).all()


def test_a_captured_call_follows_the_device_side_count(dev):
    max_rows = 70
    images_np, begins, rows, pts_np = batch_setup(dev, max_rows)
    image, pix = torch.from_numpy(images_np).to(dev), torch.from_numpy(pts_np).to(dev)
    begin = torch.from_numpy(begins).to(dev)
    count = torch.tensor((3, 4, 5), device=dev, dtype=torch.int64)
    out, valid = sentinel_rows(rows, 3, dev), torch.full((rows,), VALID_SENTINEL, device=dev, dtype=torch.uint8)

    def call():
        assert sample(pix, image, 3, 6, 9, "bgr", "hsv", 1, begin, count, max_rows, out, 3, valid) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    counts = (max_rows, 1, 33)
    count.copy_(torch.tensor(counts))
    out.view(torch.int32).fill_(SENTINEL)
    valid.fill_(VALID_SENTINEL)
    graph.replay()
    replayed = (out.cpu().numpy().view(np.int32).copy(), valid.cpu().numpy().copy())
    out.view(torch.int32).fill_(SENTINEL)
    valid.fill_(VALID_SENTINEL)
    call()
    eager = (out.cpu().numpy().view(np.int32), valid.cpu().numpy())
    exp, exp_valid = batch_expected(images_np, begins, counts, max_rows, pts_np, rows, "hsv", 1, "bgr")
    assert (replayed[0] == eager[0]).all() and (replayed[1] == eager[1]).all()
    assert (replayed[0] == exp).all() and (replayed[1] == exp_valid).all()


def test_a_cloud_that_leaves_the_buffers_is_skipped_and_flagged(dev):
    """A stale begin or count must not write out of bounds: the cloud is skipped whole, the others are served, err says so."""
    max_rows = 70
    images_np, begins, rows, pts_np = batch_setup(dev, max_rows)
    image, pix = torch.from_numpy(images_np).to(dev), torch.from_numpy(pts_np).to(dev)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    for bad_begin, counts in (((2, rows - 3, -1), (4, 4, 4)), ((2, 80, rows - max_rows + 1), (4, 4, max_rows)),
                              ((2, 80, 2 ** 62), (4, 4, 1)), ((-2 ** 62, 80, 160), (max_rows, 4, 4))):
        begin = torch.tensor(bad_begin, device=dev, dtype=torch.int64)
        count = torch.tensor(counts, device=dev, dtype=torch.int64)
        out, valid = sentinel_rows(rows, 3, dev), torch.full((rows,), VALID_SENTINEL, device=dev, dtype=torch.uint8)
        err.zero_()
        assert sample(pix, image, 3, 6, 9, "rgb", "hsv", 1, begin, count, max_rows, out, 3, valid, rows, err) == 0
        ok = [b for b in range(3) if 0 <= bad_begin[b] and bad_begin[b] + counts[b] <= rows]
        assert 0 < len(ok) < 3
        exp = np.full((rows, 3), SENTINEL, np.int32)
        exp_valid = np.full(rows, VALID_SENTINEL, np.uint8)
        for b in ok:
            lo, n = bad_begin[b], counts[b]
            c, v = R.sample_image(pts_np[lo:lo + n], images_np[b], "hsv", True, "rgb")
            exp[lo:lo + n], exp_valid[lo:lo + n] = c.view(np.int32), v
        assert (out.cpu().numpy().view(np.int32) == exp).all() and (valid.cpu().numpy() == exp_valid).all()
        assert int(err.item()) == _lib.IMAGE_ERR_ROWS
    # inside the buffers to the last row: served, no flag; and a NULL err is accepted
    begin = torch.tensor((0, 80, rows - 4), device=dev, dtype=torch.int64)
    count = torch.tensor((4, 4, 4), device=dev, dtype=torch.int64)
    err.zero_()
    assert sample(pix, image, 3, 6, 9, "rgb", "rgb", 0, begin, count, max_rows, out, 3, valid, rows, err) == 0
    assert int(err.item()) == 0
    begin[2] = rows - 3
    assert sample(pix, image, 3, 6, 9, "rgb", "rgb", 0, begin, count, max_rows, out, 3, valid, rows, None) == 0
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_output_untouched(dev):
    H, W, N = 3, 5, 8
    image = torch.zeros(2, H, W, 3, device=dev, dtype=torch.uint8) + 200
    pix = torch.zeros(N + 1, 2, device=dev, dtype=torch.int32)
    begin = torch.zeros(2, device=dev, dtype=torch.int64)
    count = torch.full((2,), N, device=dev, dtype=torch.int64)
    out = sentinel_rows(N, 4, dev)
    valid = torch.full((N,), VALID_SENTINEL, device=dev, dtype=torch.uint8)
    lib, st = _lib.load(), _lib.stream()
    good = dict(pix=p(pix), image=p(image), B=1, H=H, W=W, order=0, mode=0, norm=0, begin=None, count=None, max_rows=N, rows=N,
                out=p(out), ldo=4, valid=p(valid))
    bad = [dict(pix=None), dict(image=None), dict(out=None), dict(B=0), dict(B=65536), dict(B=2), dict(H=0), dict(W=0), dict(W=-1),
           dict(H=32768, W=32768), dict(H=1 << 15, W=21846), dict(order=2), dict(order=-1), dict(mode=2), dict(mode=-1), dict(norm=2),
           dict(norm=-1), dict(ldo=2), dict(ldo=0), dict(max_rows=-1), dict(max_rows=1 << 31), dict(begin=p(begin)),
           dict(count=p(count)), dict(pix=p(pix) + 4), dict(rows=N - 1), dict(rows=-1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.pn2_sample_image(a["pix"], a["image"], a["B"], a["H"], a["W"], a["order"], a["mode"], a["norm"], a["begin"], a["count"],
                                  a["max_rows"], a["rows"], a["out"], a["ldo"], a["valid"], None, st)
        assert rc == -1, change
    assert lib.pn2_hsv_to_rgb(p(out), 2, N, 0, p(valid), st) == -1 and lib.pn2_hsv_to_rgb(p(out), 4, -1, 0, p(valid), st) == -1
    assert lib.pn2_hsv_to_rgb(p(out), 4, N, 2, p(valid), st) == -1 and lib.pn2_hsv_to_rgb(None, 4, N, 0, p(valid), st) == -1
    assert lib.pn2_hsv_to_rgb(p(out), 4, N, 0, None, st) == -1
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENTINEL).all()) and bool((valid == VALID_SENTINEL).all())
    # the limits themselves are accepted: zero rows launch nothing, and B = 2 with both tables is a call
    assert lib.pn2_sample_image(p(pix), p(image), 1, H, W, 0, 0, 0, None, None, 0, N, p(out), 4, p(valid), None, st) == 0
    assert lib.pn2_hsv_to_rgb(None, 3, 0, 0, None, st) == 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENTINEL).all()) and bool((valid == VALID_SENTINEL).all())
    count.fill_(2)
    begin.copy_(torch.tensor((0, 4)))
    assert lib.pn2_sample_image(p(pix), p(image), 2, H, W, 0, 0, 0, p(begin), p(count), N, N, p(out), 4, p(valid), None, st) == 0
    got = out.cpu().numpy()
    assert (got[[0, 1, 4, 5], :3] == 200).all() and (got.view(np.int32)[[2, 3, 6, 7]] == SENTINEL).all()
    assert (got.view(np.int32)[:, 3] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ hsv_to_rgb
def hsv_to_rgb(rows, ld, N, order, out):
    return _lib.load().pn2_hsv_to_rgb(p(rows), ld, N, ORDER[order], p(out), _lib.stream())


def test_hsv_to_rgb_over_every_triple_of_the_forward_rule(dev):
    """All 180 x 256 x 256 (h, s, v) the forward rule can write, normalised as it normalises them; byte-equal to the fp64 statement."""
    h, s, v = np.meshgrid(np.arange(180), np.arange(256), np.arange(256), indexing="ij")
    hsv = np.stack([h.ravel(), s.ravel(), v.ravel()], -1).astype(np.float32)
    R.normalize_colors(hsv, "hsv")
    rows = torch.from_numpy(hsv).to(dev)
    N = hsv.shape[0]
    out = torch.empty(N, 3, device=dev, dtype=torch.uint8)
    assert hsv_to_rgb(rows, 3, N, "rgb", out) == 0
    want = torch.from_numpy(R.hsv_to_rgb(hsv)).to(dev)
    assert torch.equal(out, want)
    assert hsv_to_rgb(rows, 3, N, "bgr", out) == 0
    assert torch.equal(out, want.flip(-1))


def test_hsv_to_rgb_special_values_and_pitches(dev):
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    rng = np.random.RandomState(5)
    special = [[1.0, 1, 1], [below_one, 1, 1], [below_one, 0.3, 0.7], [-0.25, 1, 1], [-1e-20, 0.5, 0.5], [-3.75, 0.9, 0.2],
               [7.5, 0.4, 0.6], [np.nan, 1, 1], [0.2, np.nan, 1], [0.2, 1, np.nan], [np.inf, 1, 1], [-np.inf, 1, 1],
               [0.3, 1.5, 0.5], [0.3, -0.5, 0.5], [0.3, 0.5, 1.5], [0.3, 0.5, -0.5], [0.3, np.inf, 0.5], [0.3, 0.5, np.inf],
               [0.3, -np.inf, -np.inf], [0.0, 0.0, 0.0], [-0.0, 1.0, 1.0], [0.5, 1.0, 0.5]]
    hsv = np.concatenate([np.array(special, np.float32), rng.uniform(-2, 3, (235, 3)).astype(np.float32)])
    N = len(hsv)
    assert N == 257
    for ld in (3, 4, 7, 8):
        for order in ("rgb", "bgr"):
            for n in (1, 63, 64, 65, N):
                buf = sentinel_rows(N, ld, dev)
                buf[:, ld - 3:] = torch.from_numpy(hsv).to(dev)
                out = torch.full((N + 1, 3), VALID_SENTINEL, device=dev, dtype=torch.uint8)
                assert hsv_to_rgb(buf[:, ld - 3:], ld, n, order, out) == 0
                got = out.cpu().numpy()
                assert (got[:n] == R.hsv_to_rgb(hsv[:n], order)).all(), (ld, order, n)
                assert (got[n:] == VALID_SENTINEL).all()
    assert (R.hsv_to_rgb(hsv[7:12]) == 0).all()                      # NaN anywhere, an infinite hue: black
