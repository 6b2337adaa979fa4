"""numpy restatements of the KITTI demo's frame path (data_utils/kitti_utils.py:313-392 of the reference): the yardsticks of
tests/test_kitti_view_gpu.py.  tests/test_kitti_view_cpu.py pins ``project`` to what the reference itself returned
(tests/golden/g18_kitti_view.npz); the drawing is a plain sequential loop over the points, later points over earlier ones."""
import numpy as np

INT32_MIN = -2 ** 31


def project(pts_3d, RT, P):
    """kitti_utils.py:313-336, written out: fp64 products added left to right, each stage stored as float32, fp32 division."""
    RT, P = np.asarray(RT, np.float64), np.asarray(P, np.float64)
    x, y, z = (np.asarray(pts_3d, np.float32)[:, k].astype(np.float64) for k in range(3))
    c = [(((RT[k, 0] * x + RT[k, 1] * y) + RT[k, 2] * z) + RT[k, 3] * 1.0).astype(np.float32) for k in range(3)]
    c64 = [v.astype(np.float64) for v in c]
    q = [((P[k, 0] * c64[0] + P[k, 1] * c64[1]) + P[k, 2] * c64[2]).astype(np.float32) for k in range(3)]
    with np.errstate(all="ignore"):
        return np.stack([q[0] / q[2], q[1] / q[2]], 1)


def pixels(pts_2d):
    """``pts_2d.astype(np.int32)`` where that is defined (finite, magnitude below 2^31: truncation toward zero); INT32_MIN in
    both components of every other point."""
    pts_2d = np.asarray(pts_2d)
    with np.errstate(all="ignore"):
        ok = (np.isfinite(pts_2d) & (np.abs(pts_2d.astype(np.float64)) < 2.0 ** 31)).all(1)
    out = np.full(pts_2d.shape, INT32_MIN, np.int64)
    out[ok] = np.trunc(pts_2d[ok].astype(np.float64)).astype(np.int64)
    return out.astype(np.int32)


def top_view_pixels(pcd_3d):
    """kitti_utils.py:387-390 on ``tolist()`` floats: centres (Y, X); INT32_MIN where ``int()`` raises or leaves int32."""
    out = np.full((len(pcd_3d), 2), INT32_MIN, np.int64)
    for i, row in enumerate(np.asarray(pcd_3d, np.float32)[:, :3].tolist()):
        x, y = row[0], row[1]
        try:
            X = int(-x * 800 + 600)
            Y = int(-y * 800 + 400)
        except (ValueError, OverflowError):
            continue
        if abs(X) < 2 ** 31 and abs(Y) < 2 ** 31:
            out[i] = (Y, X)
    return out.astype(np.int32)


def draw(pix, labels, colors, size, half_widths, background=None):
    """Point after point: the rows ``dy`` of the disc, ``dx`` in ``[-hw, hw]``, clipped to the image, later points over earlier
    ones; a centre holding INT32_MIN paints nothing.  Every covered pixel then takes the colour of the last point that painted it;
    where that point's label has no colour the pixel keeps the background and the error flag is set.
    -> (image uint8 [H, W, 3], error flag)."""
    H, W = size
    img = np.zeros((H, W, 3), np.uint8) if background is None else np.array(background, np.uint8)
    r = len(half_widths) // 2
    owner = np.zeros((H, W), np.int64)
    for i, (cx, cy) in enumerate(np.asarray(pix, np.int64).tolist()):
        if cx == INT32_MIN or cy == INT32_MIN:
            continue
        for j, hw in enumerate(half_widths):
            y = cy + j - r
            if hw < 0 or not 0 <= y < H:
                continue
            x0, x1 = max(cx - hw, 0), min(cx + hw, W - 1)
            if x0 <= x1:
                owner[y, x0:x1 + 1] = i + 1
    lab = np.asarray(labels, np.int64)
    covered = owner > 0                                        # colour every covered pixel from the LAST point that painted it
    l = lab[owner[covered] - 1] if covered.any() else np.zeros(0, np.int64)
    valid = (l >= 0) & (l < len(colors))
    ys, xs = np.nonzero(covered)
    img[ys[valid], xs[valid]] = np.asarray(colors, np.uint8)[l[valid]]
    return img, int((~valid).any())


def merge(logp, groups):
    """Column-wise ``max`` of the listed members: NaN where any member is NaN, as ``Tensor.max(dim)``."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(logp))
    return torch.stack([t[..., list(m)].max(-1)[0] for m in groups], -1)
