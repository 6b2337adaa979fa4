"""numpy restatements of the 3-D ego view's rule (``pn2_depth_splat`` in include/pn2.h; ``Window_Manager.update``, pcdvis.py:31-51
of the reference): the yardsticks of tests/test_ego_view_gpu.py.  open3d is not available, so nothing here is checked against it:
the rule is the one the header states, in fp64 on the fp32 coordinates, every product and sum a separate numpy operation.

The picture is stated twice, independently: ``paint`` is a sequential painter with a depth buffer (point after point, replace iff
strictly nearer), ``per_pixel`` sorts every (pixel, depth, index) triple and keeps the first of each pixel.
tests/test_ego_view_cpu.py holds the two to each other byte for byte.  ``cloud`` builds the test inputs with their planted cases
and ``occurred`` says which of those cases an input really holds."""
import functools

import numpy as np

LIMIT = 2.0 ** 30


class Camera:
    """``E`` [3, 4] = [R | t] and ``K`` = (fx, fy, cx, cy), float64; the image is ``height`` x ``width``."""

    def __init__(self, E, K, width, height):
        self.E = np.ascontiguousarray(E, np.float64).reshape(3, 4)
        self.K = np.ascontiguousarray(K, np.float64).reshape(4)
        self.width, self.height = int(width), int(height)


def unit_camera(width, height):
    """Identity rotation, the camera 2 units behind the origin, focal length 16, principal point -0.5: a point (a*Z/16, b*Z/16,
    Z - 2) with those products exact in float32 has window coordinates (a, b) EXACTLY and depth Z exactly."""
    E = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 2.0]])
    return Camera(E, [16.0, 16.0, -0.5, -0.5], width, height)


NEAR, FAR = 1.0, 64.0                                     # the planes the planted cases are built around


def project(pts, cam, near, far):
    """-> drawn bool [N], d float32 [N], xw, yw, Z float64 [N]: steps 1 - 5 of the header's rule."""
    pts = np.asarray(pts, np.float32)
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    E, (fx, fy, cx, cy) = cam.E, cam.K
    with np.errstate(all="ignore"):
        c = [((E[k, 0] * x + E[k, 1] * y) + E[k, 2] * z) + E[k, 3] for k in range(3)]
        Z = c[2]
        drawn = (near < Z) & (Z < far)                    # (False for a NaN)
        d = Z.astype(np.float32)
        xw = ((fx * c[0]) / Z + cx) + 0.5
        yw = ((fy * c[1]) / Z + cy) + 0.5
        drawn &= np.isfinite(xw) & np.isfinite(yw)
        drawn &= (np.abs(xw) < LIMIT) & (np.abs(yw) < LIMIT)
    return drawn, d, xw, yw, Z


def first_cells(w, s):
    """First covered column (row) of a drawn point: ``floor(w + (0.5 if s is even else 0)) - s // 2`` as Python ints."""
    off = 0.5 if s % 2 == 0 else 0.0
    return [int(np.floor(v + off)) - s // 2 for v in w.tolist()]


def paint(pts, cam, s, near, far):
    """The sequential painter: -> (depth float32 [H, W], +inf empty; index int32 [H, W], -1 empty)."""
    H, W = cam.height, cam.width
    depth = np.full((H, W), np.inf, np.float32)
    index = np.full((H, W), -1, np.int32)
    drawn, d, xw, yw, _ = project(pts, cam, near, far)
    for i in np.nonzero(drawn)[0].tolist():
        x0, y0 = first_cells(xw[i:i + 1], s)[0], first_cells(yw[i:i + 1], s)[0]
        xa, xb, ya, yb = max(x0, 0), min(x0 + s, W), max(y0, 0), min(y0 + s, H)
        if xa >= xb or ya >= yb:
            continue
        win = d[i] < depth[ya:yb, xa:xb]                   # strictly less, on the float32 depth: GL_LESS in draw order
        depth[ya:yb, xa:xb][win] = d[i]
        index[ya:yb, xa:xb][win] = i
    return depth, index


def per_pixel(pts, cam, s, near, far):
    """The per-pixel statement: over all points whose square covers the pixel, the arg-min of (d, i)."""
    H, W = cam.height, cam.width
    drawn, d, xw, yw, _ = project(pts, cam, near, far)
    depth = np.full(H * W, np.inf, np.float32)
    index = np.full(H * W, -1, np.int32)
    ids = np.nonzero(drawn)[0]
    if len(ids) == 0:
        return depth.reshape(H, W), index.reshape(H, W)
    off = 0.5 if s % 2 == 0 else 0.0
    x0 = np.floor(xw[ids] + off).astype(np.int64) - s // 2
    y0 = np.floor(yw[ids] + off).astype(np.int64) - s // 2
    dy, dx = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    px = (x0[:, None] + dx.reshape(1, -1)).reshape(-1)
    py = (y0[:, None] + dy.reshape(1, -1)).reshape(-1)
    who = np.repeat(ids, s * s)
    keep = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    pixel, who = (py * W + px)[keep], who[keep]
    order = np.lexsort((who, d[who], pixel))               # by pixel, then depth, then index
    pixel, who = pixel[order], who[order]
    first = np.ones(len(pixel), bool)
    first[1:] = pixel[1:] != pixel[:-1]
    depth[pixel[first]] = d[who[first]]
    index[pixel[first]] = who[first]
    return depth.reshape(H, W), index.reshape(H, W)


def colour(index, labels, colors, background=(0, 0, 0)):
    """-> (image uint8 [H, W, 3], error flag): ``colors[labels[index]]`` where a point is visible and its label has a colour,
    else the background (a triple or an image); the flag is 1 if a visible point's label lies outside ``[0, C)``."""
    H, W = index.shape
    bg = np.asarray(background, np.uint8)
    img = np.array(np.broadcast_to(bg, (H, W, 3)), np.uint8)
    seen = index >= 0
    l = np.asarray(labels, np.int64)[index[seen]]
    valid = (l >= 0) & (l < len(colors))
    ys, xs = np.nonzero(seen)
    img[ys[valid], xs[valid]] = np.asarray(colors, np.uint8)[l[valid]]
    return img, int((~valid).any())


# ------------------------------------------------------------------------------------------------------------------- inputs
def at(a, b, Z):
    """The point of ``unit_camera`` whose window coordinates are (a, b) and whose depth is Z (exactly, where a*Z/16 is exact)."""
    return [a * Z / 16.0, b * Z / 16.0, Z - 2.0]


def planted(W, H):
    """Points for ``unit_camera(W, H)`` with planes (NEAR, FAR) that decide every rule, in a fixed order."""
    f32 = np.float32
    nan, inf = float("nan"), float("inf")
    tiny = float(f32(1e-3))
    tinier = float(np.nextafter(f32(1e-3), f32(0)))
    p = []
    p += [at(10.3, 10.3, 4.0), at(10.3, 10.3, 2.0)]                      # one pixel, the nearer point second ...
    p += [at(20.3, 10.3, 2.0), at(20.3, 10.3, 4.0)]                      # ... and first
    p += [at(30.3, 10.3, 3.0)] * 3                                       # exact duplicates
    # fp64 depths 2 + 1e-3 and a hair less, one float32 depth: the FIRST is the farther in fp64 and must still win
    p += [[40.3 / 8, 10.3 / 8, tiny], [40.3 / 8, 10.3 / 8, tinier]]
    near_up, near_down = float(np.nextafter(f32(-1), f32(0))), float(np.nextafter(f32(-1), f32(-2)))
    for z in (-1.0, near_down, -3.0, -2.0, nan, inf, -inf, 62.0, 100.0, 3e38):     # Z = near, below, negative, 0, NaN, inf, >= far
        p.append([15.3 / 8, 20.3 / 8, z])
    p.append([16.3 / 16, 24.3 / 16, near_up])                            # just inside the near plane: drawn
    p.append([17.3 * 4, 24.3 * 4, float(np.nextafter(f32(62), f32(0)))])  # just inside the far plane: drawn
    big = 2.0 ** 27                                                      # 16 * 2^27 / 2 = 2^30: the first centre that is skipped
    p += [[1e30, 0, 0], [-1e30, 0, 0], [0, 1e30, 0], [0, -1e30, 0], [1e30, 1e30, 1e30], [3e38, -3e38, 0],
          [big, 0, 0], [-big, 0, 0], [0, big, 0], [0, -big, 0],
          [float(np.nextafter(f32(big), f32(0))), 1.0, 0], [1.0, float(np.nextafter(f32(-big), f32(0))), 0],
          [-0.0, -0.0, 0.0], [-0.0, 1.0, -0.0], [inf, 0, 0], [0, -inf, 0], [nan, 0, 0], [0, nan, 0]]
    for k in (7.0, 7.5, 0.0, 0.5, W - 1.0, W - 0.5, float(W)):           # window coordinates exactly on k and on k + 0.5
        p.append(at(k, 20.0, 2.0))
    for k in (20.0, 20.5, 0.0, 0.5, H - 1.0, H - 0.5, float(H)):
        p.append(at(33.0, k, 2.0))
    sweep = np.arange(-4.0, 4.01, 0.5).tolist()                          # squares across, at and beyond every edge and corner
    for e in sweep:
        p += [at(e, 15.25, 2.0), at(W + e, 15.25, 2.0), at(25.25, e, 2.0), at(25.25, H + e, 2.0)]
    for ex in (-2.5, -1.0, -0.5, 0.0, 0.5, 1.0, 2.5):
        p += [at(ex, ex, 4.0), at(W + ex, ex, 4.0), at(ex, H + ex, 4.0), at(W + ex, H + ex, 4.0)]
    return np.array(p, np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cloud(N, W, H):
    """float32 [N, 3] for ``unit_camera(W, H)``: the planted points first, then random ones with window coordinates up to 3 pixels
    outside the image and depths from a handful of values, so that float32 depth ties between different points are common."""
    fixed = planted(W, H)
    if N <= len(fixed):
        pts = fixed[:N]
    else:
        rng = np.random.default_rng(1000 * N + W)
        n = N - len(fixed)
        Z = rng.choice([1.5, 2.0, 2.0, 2.25, 3.0, 5.0, 40.0], n)
        a, b = rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n)
        half = rng.random(n) < 0.2                                       # a fifth sit on multiples of a quarter pixel
        a[half], b[half] = np.round(a[half] * 4) / 4, np.round(b[half] * 4) / 4
        rand = np.stack([a * Z / 16.0, b * Z / 16.0, Z - 2.0], 1).astype(np.float32)
        if n >= 8:
            rand[n // 2:n // 2 + 4] = rand[:4]                           # duplicates among the random points too
        pts = np.concatenate([fixed, rand], 0)
    pts = np.ascontiguousarray(pts, np.float32).reshape(N, 3)
    pts.setflags(write=False)
    return pts


def occurred(pts, cam, s, near, far):
    """Which of the planted situations the input really holds, read off the restatement's own numbers: a dict of booleans
    (a one-pixel point cannot be clipped: those entries are True at ``s == 1``)."""
    H, W = cam.height, cam.width
    drawn, d, xw, yw, Z = project(pts, cam, near, far)
    ids = np.nonzero(drawn)[0]
    x0 = np.array(first_cells(xw[ids], s), np.int64)
    y0 = np.array(first_cells(yw[ids], s), np.int64)
    cell = {}
    for k, i in enumerate(ids.tolist()):
        cell.setdefault((int(x0[k]), int(y0[k])), []).append(i)
    inside = lambda c: 0 <= c[0] and c[0] + s <= W and 0 <= c[1] and c[1] + s <= H
    near_second = near_first = dup = tie = False
    for c, members in cell.items():
        if not inside(c):
            continue
        for a in range(len(members)):
            for b in range(a + 1, len(members)):
                i, j = members[a], members[b]
                near_second |= bool(d[j] < d[i])
                near_first |= bool(d[i] < d[j])
                dup |= bool((np.asarray(pts)[i, :3].view(np.uint32) == np.asarray(pts)[j, :3].view(np.uint32)).all())
                tie |= bool(d[i] == d[j] and Z[j] < Z[i])
    frac_x, frac_y = xw[ids] - np.floor(xw[ids]), yw[ids] - np.floor(yw[ids])
    x1, y1 = x0 + s - 1, y0 + s - 1
    return {
        "nearer point second": near_second, "nearer point first": near_first, "exact duplicates": dup,
        "equal float32 depth, different fp64 depth": tie,
        "Z == near": bool((Z == near).any()), "Z just below near": bool(((Z < near) & (Z > near - 1e-6)).any()),
        "Z negative": bool((Z < 0).any()), "Z zero": bool((Z == 0).any()), "Z NaN": bool(np.isnan(Z).any()),
        "Z +inf": bool((Z == np.inf).any()), "Z == far": bool((Z == far).any()), "Z beyond far": bool((Z > far).any()),
        "centre at 2^30": bool(((np.abs(xw) == LIMIT) | (np.abs(yw) == LIMIT)).any()),
        "centre beyond 2^30": bool((np.isfinite(xw) & (np.abs(xw) > 1e20)).any() and (np.isfinite(yw) & (np.abs(yw) > 1e20)).any()),
        "centre just below 2^30": bool((drawn & ((np.abs(xw) > LIMIT / 2) | (np.abs(yw) > LIMIT / 2))).any()),
        "negative zero": bool((np.signbit(np.asarray(pts)[:, :3]) & (np.asarray(pts)[:, :3] == 0)).any()),
        "x on k": bool((frac_x == 0).any()), "x on k + 0.5": bool((frac_x == 0.5).any()),
        "y on k": bool((frac_y == 0).any()), "y on k + 0.5": bool((frac_y == 0.5).any()),
        "clipped left": s == 1 or bool(((x0 < 0) & (x1 >= 0) & (y0 >= 0) & (y1 < H)).any()),
        "clipped right": s == 1 or bool(((x0 < W) & (x1 >= W) & (y0 >= 0) & (y1 < H)).any()),
        "clipped top": s == 1 or bool(((y0 < 0) & (y1 >= 0) & (x0 >= 0) & (x1 < W)).any()),
        "clipped bottom": s == 1 or bool(((y0 < H) & (y1 >= H) & (x0 >= 0) & (x1 < W)).any()),
        "clipped corners": s == 1 or all(bool((cx & cy).any()) for cx in ((x0 < 0) & (x1 >= 0), (x0 < W) & (x1 >= W))
                               for cy in ((y0 < 0) & (y1 >= 0), (y0 < H) & (y1 >= H))),
        "one pixel outside": bool((x1 == -1).any() and (x0 == W).any() and (y1 == -1).any() and (y0 == H).any()),
    }


@functools.lru_cache(maxsize=None)
def reference(N, W, H, s):
    """(depth, index) of ``cloud(N, W, H)`` through ``unit_camera(W, H)`` at point size ``s``, read-only, computed once."""
    depth, index = paint(cloud(N, W, H), unit_camera(W, H), s, NEAR, FAR)
    depth.setflags(write=False)
    index.setflags(write=False)
    return depth, index
