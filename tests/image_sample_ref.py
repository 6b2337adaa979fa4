"""numpy statements of the camera colour lookup (csrc/image.hip, include/pn2.h) and of the colour-generation task's window:

  * ``hsv_u8``            the integer HSV rule (OpenCV's 8-bit BGR2HSV as include/pn2.h states it; UNVERIFIED against OpenCV);
  * ``hsv_real``          the real-valued definition it is held to on the CPU;
  * ``sample_loop``       the lookup one point at a time, the way of data_utils/ColorGenerator_Loader.py:59-69 (restated; a Python loop);
  * ``sample_image``      the same, vectorised (what the GPU tests compare with);
  * ``hsv_to_rgb``        the way back, in fp64;
  * ``window_rows``       the rows ``ColorGeneratorLoader.__getitem__`` (:89-100) returns, and ``window_item``, that
    method's cut restated.
"""
import numpy as np

INT32_MIN = -2 ** 31


def hsv_tables():
    """sdiv[i] = rint(255 * 4096 / i), hdiv[i] = rint(180 * 4096 / (6 i)): round-half-even in fp64, both 0 at i = 0."""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
    sdiv[1:] = np.rint(255.0 * 4096.0 / i).astype(np.int64)
    hdiv[1:] = np.rint(180.0 * 4096.0 / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


SDIV, HDIV = hsv_tables()


def hsv_u8(r, g, b):
    """(h, s, v) int64 arrays of integer channel arrays: the rule of include/pn2.h."""
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = (d * SDIV[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * HDIV[d] + 2048) >> 12                                   # (numpy's >> on signed integers is arithmetic)
    return np.where(h < 0, h + 180, h), s, v


def hsv_real(r, g, b):
    """The real-valued definition in OpenCV's 8-bit units: (hue in [0, 180), saturation 255 d / v), float64; hue = 30 * sector with
    sector = (g - b) / d, 2 + (b - r) / d or 4 + (r - g) / d for the maximum r, g, b (tested in that order), wrapped; 0 for a grey."""
    r, g, b = (np.asarray(c).astype(np.float64) for c in (r, g, b))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    dd = np.where(d == 0, 1.0, d)
    sector = np.where(v == r, (g - b) / dd, np.where(v == g, 2.0 + (b - r) / dd, 4.0 + (r - g) / dd))
    hue = np.where(d == 0, 0.0, np.mod(30.0 * sector, 180.0))
    sat = np.where(v == 0, 0.0, 255.0 * d / np.where(v == 0, 1.0, v))
    return hue, sat


def color_frame(image, mode, channel_order):
    """float32 [H, W, 3] of a uint8 [H, W, 3] image: (R, G, B) or (H, S, V) per pixel -- the reference's ``frame`` / ``frame_HSV``."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    c0, c1, c2 = image[..., 0], image[..., 1], image[..., 2]
    r, g, b = (c2, c1, c0) if channel_order == "bgr" else (c0, c1, c2)
    assert channel_order in ("rgb", "bgr") and mode in ("rgb", "hsv")
    planes = hsv_u8(r, g, b) if mode == "hsv" else (r, g, b)
    return np.stack([np.asarray(p).astype(np.float32) for p in planes], -1)


def normalize_colors(pts_color, mode):
    """ColorGenerator_Loader.py:68-69, numpy's in-place float32 divisions (for RGB every column by 255)."""
    assert pts_color.dtype == np.float32
    if mode == "hsv":
        pts_color[:, 0] /= 180
        pts_color[:, 1:] /= 255
    else:
        pts_color /= 255
    return pts_color


def sample_loop(pix, image, mode="rgb", normalize=True, channel_order="rgb"):
    """The lookup one point at a time, as the reference goes about it (data_utils/ColorGenerator_Loader.py:59-69; restated, not
    copied): a point whose truncated pixel lies in the frame takes that pixel's colour, every other point keeps zeros; the
    normalising divisions run once over the finished array.  The reference's loop names its unpacked pair ``(y, x)`` with ``y`` the
    COLUMN; here the pair is (column, row).  -> (colors float32 [M, 3], valid bool [M])."""
    pixels = np.asarray(pix, np.int32)
    frame = color_frame(image, mode, channel_order)
    rows, cols = frame.shape[:2]
    colors = np.zeros((len(pixels), 3), np.float32)
    valid = np.zeros(len(pixels), bool)
    for n in range(len(pixels)):
        col, row = int(pixels[n, 0]), int(pixels[n, 1])
        if 0 <= row < rows and 0 <= col < cols:
            colors[n] = frame[row, col]
            valid[n] = True
    return (normalize_colors(colors, mode) if normalize else colors), valid


def sample_image(pix, image, mode="rgb", normalize=True, channel_order="rgb"):
    """The vectorised statement: pix int32 [M, 2] (x = column, y = row), image uint8 [H, W, 3] -> (float32 [M, 3], bool [M])."""
    pix = np.asarray(pix, np.int32).astype(np.int64)
    frame = color_frame(image, mode, channel_order)
    H, W = frame.shape[:2]
    x, y = pix[:, 0], pix[:, 1]
    valid = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    out = np.zeros((pix.shape[0], 3), np.float32)
    out[valid] = frame[y[valid], x[valid]]
    if normalize:
        normalize_colors(out, mode)
    return out, valid


def hsv_to_rgb(hsv, channel_order="rgb"):
    """uint8 [N, 3] of float32 [N, 3] normalised (h, s, v): the fp64 rule of include/pn2.h (pn2_hsv_to_rgb), every operation a
    separately rounded numpy float64 operation."""
    hsv = np.asarray(hsv, np.float32).astype(np.float64).reshape(-1, 3)
    h, s, v = hsv[:, 0], hsv[:, 1], hsv[:, 2]
    with np.errstate(invalid="ignore"):
        h6 = (h - np.floor(h)) * 6.0
        black = np.isnan(h6) | np.isnan(s) | np.isnan(v)
        s = np.clip(np.where(black, 0.0, s), 0.0, 1.0)
        v = np.clip(np.where(black, 0.0, v), 0.0, 1.0)
        h6 = np.where(black, 0.0, h6)
        k = np.minimum(h6.astype(np.int64), 5)
        f = h6 - k.astype(np.float64)
        p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    rgb = np.stack([np.rint(255.0 * c) for c in (r, g, b)], -1)
    rgb[black] = 0.0
    rgb = rgb.astype(np.uint8)
    return np.ascontiguousarray(rgb[:, ::-1]) if channel_order == "bgr" else rgb


def window_rows(length, npoints, start):
    """The rows of the cloud an item holds: ``(start + i) % length`` (start = 0 unless the cloud is longer than the window)."""
    return (int(start) + np.arange(npoints, dtype=np.int64)) % int(length)


def window_item(pcd, label, npoints):
    """The item ``ColorGeneratorLoader.__getitem__`` cuts from a cloud of L rows (ColorGenerator_Loader.py:89-101; restated, not
    copied): L == npoints, the cloud itself; L > npoints, the rows [start, start + npoints) with start = np.random.randint(0, L -
    npoints), the one draw; L < npoints, the cloud followed by its own first npoints - L rows -- of which there are only L, so a
    cloud shorter than half the window gives a SHORT item of 2 L rows, as in the reference."""
    L = len(pcd)
    if L > npoints:
        start = np.random.randint(0, L - npoints)
        return pcd[start:start + npoints], label[start:start + npoints]
    if L < npoints:
        return np.concatenate([pcd, pcd[:npoints - L]]), np.concatenate([label, label[:npoints - L]])
    return pcd, label
