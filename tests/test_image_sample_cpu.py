"""CPU: the statements of tests/image_sample_ref.py hold what include/pn2.h says of pn2_sample_image, and can tell a wrong kernel
from a right one (the mutants below).  No GPU, no library call."""
import numpy as np
import pytest

import image_sample_ref as R

INT32_MIN = R.INT32_MIN


# ------------------------------------------------------------------------------------------------------- the integer HSV rule
def test_hsv_rule_against_the_real_valued_definition_over_all_colours():
    """Caps are conditions, not measurements: hue within 0.65 (circular) of 30 * sector, saturation within 0.53 of 255 d / v,
    h in 0 .. 179, s in 0 .. 255.  (The rule itself gives 0.640 and 0.522.)"""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    g, b = g.ravel(), b.ravel()
    worst_h = worst_s = 0.0
    for r in range(256):
        rr = np.full_like(g, r)
        h, s, v = R.hsv_u8(rr, g, b)
        hue, sat = R.hsv_real(rr, g, b)
        assert h.min() >= 0 and h.max() <= 179 and s.min() >= 0 and s.max() <= 255
        assert (v == np.maximum(rr, np.maximum(g, b))).all()
        dh = np.abs(h - hue)
        worst_h = max(worst_h, float(np.minimum(dh, 180.0 - dh).max()))
        worst_s = max(worst_s, float(np.abs(s - sat).max()))
    print("hue error %.4f, saturation error %.4f" % (worst_h, worst_s))
    assert worst_h <= 0.65 and worst_s <= 0.53


def test_tables_are_what_the_header_states():
    assert R.SDIV[0] == 0 and R.HDIV[0] == 0
    assert R.SDIV[255] == 4096 and R.SDIV[1] == 255 * 4096 and R.HDIV[1] == 30 * 4096
    assert R.SDIV[2] == 522240 and R.HDIV[60] == 2048        # exact quotients; 255 * 4096 / 2 is no tie


# --------------------------------------------------------------------------------------------------- a float32 restatement
def restate(pix, image, mode, normalize, channel_order, mutant=None):
    """pn2_sample_image's rule once more, point by point, in numpy float32 scalars; ``mutant`` plants one mistake."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    f32 = np.float32
    out = np.zeros((len(pix), 3), f32)
    valid = np.zeros(len(pix), bool)
    for i, (x, y) in enumerate(np.asarray(pix).tolist()):
        if mutant == "swap":
            x, y = y, x
        inside = (0 <= y <= H and 0 <= x <= W) if mutant == "far_le" else (0 <= y < H and 0 <= x < W)
        if not inside:
            continue
        valid[i] = True
        c = [int(t) for t in image[y % H, x % W]]                     # (% only matters to the far_le mutant)
        r, g, b = (c[2], c[1], c[0]) if (channel_order == "bgr" and mutant != "order_ignored") else c
        if mode == "rgb":
            vals, div = [r, g, b], [255, 255, 255]
        else:
            v = max(r, g, b)
            d = v - min(r, g, b)
            s = (d * int(R.SDIV[v]) + 2048) >> 12
            if mutant == "g_first":
                h0 = b - r + 2 * d if v == g else (g - b if v == r else r - g + 4 * d)
            else:
                h0 = g - b if v == r else (b - r + 2 * d if v == g else r - g + 4 * d)
            h = (h0 * int(R.HDIV[d]) + 2048) >> 12                    # (Python's >> on a negative int is arithmetic)
            if h < 0 and mutant != "no180":
                h += 180
            vals, div = [h, s, v], [180, 255, 255]
        for k in range(3):
            q = f32(vals[k])
            if normalize:
                q = q * (f32(1) / f32(div[k])) if mutant == "recip" else q / f32(div[k])
            out[i, k] = q
    return out, valid


def border_points(H, W):
    """Every pixel of the image, the ring around it, and the unprojectable marker in one and in both components."""
    pts = [(x, y) for y in range(-2, H + 2) for x in range(-2, W + 2)]
    pts += [(INT32_MIN, INT32_MIN), (INT32_MIN, 0), (0, INT32_MIN), (2 ** 31 - 1, 0), (0, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1)]
    return np.array(pts, np.int32)


def cases():
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, (7, 5, 3)).astype(np.uint8)
    img[..., 2] = 255 - img[..., 0] // 2                              # R != B everywhere: the channel order always shows
    pts = border_points(7, 5)
    # one row of colours whose hue is negative before the wrap (maximum R, G < B), and one of all 256 grey / hue levels
    neg = np.array([[[200, 10, 90], [255, 0, 255], [90, 3, 4], [17, 0, 16]]], np.uint8)
    lev = np.stack([np.arange(256), (np.arange(256) * 7) % 256, (np.arange(256) * 13 + 5) % 256], -1).astype(np.uint8)[None]
    row = lambda n: np.stack([np.arange(n), np.zeros(n, int)], -1).astype(np.int32)
    return {
        "border_rgb_raw": (pts, img, "rgb", False, "rgb"),
        "border_hsv_norm_bgr": (pts, img, "hsv", True, "bgr"),
        "negative_hue": (row(4), neg, "hsv", False, "rgb"),
        "levels_rgb_norm": (row(256), lev, "rgb", True, "rgb"),
        "levels_hsv_norm": (row(256), lev, "hsv", True, "rgb"),
    }


# the cases each mutant can affect (the others it must leave alone: that is checked as well)
AFFECTS = {
    "swap": {"border_rgb_raw", "border_hsv_norm_bgr"},                # (the one-row images are read at y = 0: a swap leaves the frame)
    "far_le": {"border_rgb_raw", "border_hsv_norm_bgr"},
    "order_ignored": {"border_hsv_norm_bgr"},
    "no180": {"border_hsv_norm_bgr", "negative_hue", "levels_hsv_norm"},
    "recip": {"border_hsv_norm_bgr", "levels_rgb_norm", "levels_hsv_norm"},
    "g_first": set(),
}


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all()


def test_vectorised_statement_equals_the_transcribed_loop():
    for name, (pix, img, mode, norm, order) in cases().items():
        assert same(R.sample_image(pix, img, mode, norm, order), R.sample_loop(pix, img, mode, norm, order)), name
    pix, img = cases()["border_rgb_raw"][:2]
    colors, valid = R.sample_loop(pix, img, "rgb", False, "rgb")
    assert valid.sum() == 7 * 5 and not valid[-6:].any()
    assert (colors[~valid] == 0).all() and not np.signbit(colors[~valid]).any()


def test_float32_restatement_passes():
    for name, (pix, img, mode, norm, order) in cases().items():
        assert same(restate(pix, img, mode, norm, order), R.sample_image(pix, img, mode, norm, order)), name


@pytest.mark.parametrize("mutant", ["swap", "far_le", "order_ignored", "no180", "recip"])
def test_mutants_fail_on_every_case_they_can_affect(mutant):
    for name, (pix, img, mode, norm, order) in cases().items():
        if mutant == "swap" and name not in AFFECTS[mutant]:
            continue                                                  # a swapped read of a one-row image is out of its bounds
        equal = same(restate(pix, img, mode, norm, order, mutant), R.sample_image(pix, img, mode, norm, order))
        assert equal == (name not in AFFECTS[mutant]), (mutant, name)


def test_the_order_of_the_r_and_g_tests_cannot_show():
    """Testing ``v == g`` before ``v == r`` only differs where r == g == v, and there g - b == b - r + 2 d == d: the order the header
    states is OpenCV's, but no colour can tell it from the other.  Held over all 2^24 colours, so a kernel written either way passes
    the same tests."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for r in range(256):
        rr = np.full_like(g, r)
        v = np.maximum(rr, np.maximum(g, b))
        d = v - np.minimum(rr, np.minimum(g, b))
        first_r = np.where(v == rr, g - b, np.where(v == g, b - rr + 2 * d, rr - g + 4 * d))
        first_g = np.where(v == g, b - rr + 2 * d, np.where(v == rr, g - b, rr - g + 4 * d))
        assert (first_r == first_g).all()
    for name, (pix, img, mode, norm, order) in cases().items():
        assert same(restate(pix, img, mode, norm, order, "g_first"), R.sample_image(pix, img, mode, norm, order)), name


# ------------------------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("length", ["n", "n+1", "2n", "n-1", "n/2", "3"])
def test_window_choice_equals_getitem_index_arithmetic(length):
    from pointnet12_amd import loader
    npoints = 16
    length = {"n": npoints, "n+1": npoints + 1, "2n": 2 * npoints, "n-1": npoints - 1, "n/2": npoints // 2, "3": 3}[length]
    pcd = np.arange(length * 4, dtype=np.float32).reshape(length, 4)
    label = np.arange(length * 3, dtype=np.float32).reshape(length, 3) + 0.5
    for seed in range(5):
        np.random.seed(seed)
        want_p, want_l = R.window_item(pcd, label, npoints)
        after = np.random.randint(1 << 30)
        np.random.seed(seed)
        rows = R.window_rows(length, npoints, loader.color_window_start(length, npoints))
        assert np.random.randint(1 << 30) == after                   # the same draws were consumed
        if 2 * length >= npoints:
            assert (pcd[rows] == want_p).all() and (label[rows] == want_l).all()
        else:
            # the reference returns a SHORT item here (2 * length rows) and fails at collate; the wrap continues it
            assert want_p.shape[0] == 2 * length < npoints
            assert (pcd[rows][:2 * length] == want_p).all() and (label[rows][:2 * length] == want_l).all()
            assert (rows == np.arange(npoints) % length).all()


def test_hsv_to_rgb_statement_on_known_colours():
    hsv = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [60 / 180, 1, 1], [120 / 180, 1, 1], [1.0, 1, 1], [-1e-20, 1, 1],
                    [0.5, 2.0, -1.0], [np.nan, 1, 1], [0, np.nan, 1], [np.inf, 1, 1], [30 / 180, 1, 1]], np.float32)
    want = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 0, 0], [255, 0, 0],
            [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [255, 255, 0]]
    got = R.hsv_to_rgb(hsv)
    assert got.tolist() == want
    assert (R.hsv_to_rgb(hsv, "bgr") == got[:, ::-1]).all()


def test_colorgen_has_the_segmentation_networks_state_keys():
    from pointnet12_amd import pointnet as P
    for ft in (False, True):
        a, b = P.PointNetColorGen(3, 4, ft).state_dict(), P.PointNetSeg(3, 4, ft).state_dict()
        assert list(a.keys()) == list(b.keys())
        assert [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]


def test_refusals_need_no_gpu():
    """Bad arguments return PN2_EINVAL before any launch (the pointers below are never dereferenced)."""
    from pointnet12_amd import _lib
    lib = _lib.load()
    good = [64, 64, 1, 4, 4, 0, 0, 0, None, None, 0, 0, 64, 3, None, None, None]  # max_rows = 0: accepted, nothing launched
    assert lib.pn2_sample_image(*good) == 0
    for at, value in ((0, None), (1, None), (12, None), (2, 0), (2, 65536), (2, 2), (3, 0), (4, 0), (5, 2), (6, 2), (7, 2), (13, 2),
                      (10, -1), (10, 1 << 31), (10, 1), (11, -1), (8, 64), (9, 64), (0, 68)):        # (10, 1): rows < max_rows
        args = list(good)
        args[at] = value
        assert lib.pn2_sample_image(*args) == -1, (at, value)
    args = list(good)
    args[3], args[4] = 1 << 15, 21846                                # H * W * 3 = 2^31 + 65 536
    assert lib.pn2_sample_image(*args) == -1
    assert lib.pn2_hsv_to_rgb(None, 3, 0, 0, None, None) == 0
    for args in ((64, 2, 0, 0, 64, None), (64, 3, -1, 0, 64, None), (64, 3, 0, 2, 64, None), (None, 3, 1, 0, 64, None),
                 (64, 3, 1, 0, None, None)):
        assert lib.pn2_hsv_to_rgb(*args) == -1, args
