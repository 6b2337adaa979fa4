"""The rule of include/pn2.h ("segment boxes") in numpy: what pn2_segment_boxes must write, bit for bit.

float32 arrays throughout, so numpy rounds every operation on its own; ``np.fmin`` / ``np.fmax`` stand for fminf / fmaxf; minima and
maxima are taken in the total order of the order-preserving uint32 key (-0.0 < +0.0).  The loop is per segment; the angles of the
table are one array axis (each angle's arithmetic is still its own chain of float32 operations)."""
import math

import numpy as np

ERR_RANGE, ERR_NONFINITE = 1024, 2048            # PN2_BOX_ERR_* of include/pn2.h
MAX_XY = np.float32(2.0 ** 60)
SCALE = np.float32(1048576.0)


def angle_table(A):
    """float32 [A, 4]: (cos, sin, theta, 0) of theta_a = a * (pi / 2) / A, computed in fp64 and rounded once."""
    theta = np.arange(A, dtype=np.float64) * (math.pi / 2) / A
    t = np.zeros((A, 4), np.float32)
    t[:, 0], t[:, 1], t[:, 2] = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32), theta.astype(np.float32)
    return t


def key(f):
    b = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def kmin(f, axis=-1):
    return unkey(key(f).min(axis=axis))


def kmax(f, axis=-1):
    return unkey(key(f).max(axis=axis))


def takes_part(points, axes):
    cx, cy, cz = axes
    with np.errstate(invalid="ignore"):
        return (np.abs(points[:, cx]) <= MAX_XY) & (np.abs(points[:, cy]) <= MAX_XY) & np.isfinite(points[:, cz])


def fit(x, y, table, d0):
    """One segment's rows (float32, all taking part, at least one) -> (angle, score, u0, u1, v0, v1 of the winner, area [A], scores [A])."""
    c, s = table[:, 0:1], table[:, 1:2]                              # [A, 1]
    x, y = x[None, :], y[None, :]
    u = (c * x) + (s * y)                                            # [A, n], each operation rounded to float32
    v = (c * y) - (s * x)
    u0, u1, v0, v1 = kmin(u), kmax(u), kmin(v), kmax(v)
    lu, lv = u1 - u0, v1 - v0
    area = lu * lv
    d0 = np.float32(d0)
    if d0 > 0:
        e = np.fmin(np.fmin(u - u0[:, None], u1[:, None] - u), np.fmin(v - v0[:, None], v1[:, None] - v))
        d = np.fmax(e, d0)
        q = d0 / d
        t = (q * SCALE).astype(np.int32)                             # exact product; the conversion truncates
        scores = t.astype(np.int64).sum(axis=1)
    else:
        scores = np.zeros(len(table), np.int64)
    best = 0
    for a in range(1, len(table)):                                   # ascending, replace on strict improvement
        if scores[a] > scores[best] or (scores[a] == scores[best] and area[a] < area[best]):
            best = a
    return best, int(scores[best]), u0[best], u1[best], v0[best], v1[best], area, scores


def segment_boxes(points, seg, count, table, d0=0.05, axes=(0, 1, 2)):
    """pn2_segment_boxes on ONE cloud: points float32 [rows, ld], seg int [rows], ``count`` segments.  Returns a dict of arrays with one
    row per segment (center / size / lo / hi float32 [count, 3], yaw float32, angle / n int32, score int64) and ``err``."""
    points = np.ascontiguousarray(points, np.float32)
    seg = np.asarray(seg).astype(np.int64)
    table = np.ascontiguousarray(table, np.float32)
    cx, cy, cz = axes
    out = {"center": np.zeros((count, 3), np.float32), "size": np.zeros((count, 3), np.float32), "yaw": np.zeros(count, np.float32),
           "angle": np.full(count, -1, np.int32), "lo": np.zeros((count, 3), np.float32), "hi": np.zeros((count, 3), np.float32),
           "n": np.zeros(count, np.int32), "score": np.zeros(count, np.int64), "err": 0}
    if (seg >= count).any():
        out["err"] |= ERR_RANGE
    named = (seg >= 0) & (seg < count)
    ok = takes_part(points, axes)
    if (named & ~ok).any():
        out["err"] |= ERR_NONFINITE
    half = np.float32(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(count):
            rows = points[named & ok & (seg == s)]
            if len(rows) == 0:
                continue
            x, y, z = rows[:, cx], rows[:, cy], rows[:, cz]
            a, score, u0, u1, v0, v1, _, _ = fit(x, y, table, d0)
            c, sn = table[a, 0], table[a, 1]
            z0, z1 = kmin(z), kmax(z)
            cu, cv = half * (u0 + u1), half * (v0 + v1)
            out["center"][s] = ((c * cu) - (sn * cv), (sn * cu) + (c * cv), half * (z0 + z1))
            out["size"][s] = (u1 - u0, v1 - v0, z1 - z0)
            out["yaw"][s], out["angle"][s], out["n"][s], out["score"][s] = table[a, 2], a, len(rows), score
            out["lo"][s] = (kmin(x), kmin(y), z0)
            out["hi"][s] = (kmax(x), kmax(y), z1)
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def car_l_shape(rng, n, yaw, centre=(12.0, 0.0), length=4.2, width=1.8, sigma=0.02):
    """n points on the two sides of a length x width rectangle that a sensor at the origin sees (an L), heading ``yaw`` (radians),
    Gaussian noise sigma; float32 [n, 3] with z in [0, 1.5]."""
    corners = np.array([[length / 2, width / 2], [-length / 2, width / 2], [-length / 2, -width / 2], [length / 2, -width / 2]])
    R = np.array([[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]])
    world = corners @ R.T + np.asarray(centre)
    near = int(np.argmin((world ** 2).sum(1)))                       # the corner nearest the sensor: its two sides are seen
    a, b, c = world[(near - 1) % 4], world[near], world[(near + 1) % 4]
    la, lc = np.linalg.norm(a - b), np.linalg.norm(c - b)
    on_a = rng.random(n) < la / (la + lc)
    t = rng.random(n)[:, None]
    xy = np.where(on_a[:, None], b + t * (a - b), b + t * (c - b)) + rng.normal(scale=sigma, size=(n, 2))
    return np.concatenate([xy, rng.uniform(0.0, 1.5, (n, 1))], 1).astype(np.float32)


def yaw_error_deg(yaw, truth):
    """The heading error modulo a quarter turn, in degrees (both arguments in radians)."""
    d = (math.degrees(float(yaw) - float(truth)) + 45.0) % 90.0 - 45.0
    return abs(d)
