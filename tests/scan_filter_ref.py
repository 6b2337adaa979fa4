"""numpy restatement of the device scan filter's rule (include/pn2.h, ``pn2_scan_filter``), for the tests.

The rule: ``sem = word & 0xFFFF``, ``c = lut[sem]``, kept only if ``c > 0``, output class ``c - 1``; ``d`` in float32 exactly as
``np.sqrt(x**2 + y**2 + z**2)``; the eight strict float32 box comparisons; the two angles as FP64 ``arctan2`` values rounded to
float32 and compared, strictly, with float32 thresholds; kept rows in scan order.

It differs from the reference (``kitti.in_view``: numpy's float32 ``arctan2``) only where an angle lies within a few float32
steps of a threshold.  ``undecided`` marks those points: ``|a64 - float64(t)| <= w * np.spacing(np.float32(|t|))`` for an active
threshold ``t`` and the point's fp64 angle ``a64``.  ``w = 4`` is the band for comparisons with the reference's float32
``arctan2`` (it is off the rounded fp64 value by at most 3 ulp: tests/test_scan_filter_cpu.py counts it), ``w = 1`` the band for
comparisons of the device with this restatement (two fp64 ``atan2`` implementations differ in their last bits only).
"""
import numpy as np

DEFAULT_BOX = (-10000, 10000) * 4


def thresholds(h_fov=(-40, 40), v_fov=(-20, 20)):
    """float32 ``[t0, t1, t2, t3]``: ``t0 < az < t1``, ``t2 < el < t3`` -- the reference's expressions (kitti_utils.py:243-247)."""
    return np.array([-h_fov[1] * np.pi / 180, -h_fov[0] * np.pi / 180, v_fov[0] * np.pi / 180, v_fov[1] * np.pi / 180],
                    np.float64).astype(np.float32)


def make_lut(learning_map):
    lut = np.full(int(max(learning_map)) + 1, -1, np.int32)
    for k, v in learning_map.items():
        lut[int(k)] = int(v)
    return lut


def angles64(points):
    """(d float32, az fp64, el fp64) of rows ``[M, >= 3]`` float32."""
    x, y, z = (np.ascontiguousarray(points[:, k], np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        d = np.sqrt(x ** 2 + y ** 2 + z ** 2)
    return d, np.arctan2(y.astype(np.float64), x.astype(np.float64)), np.arctan2(z.astype(np.float64), d.astype(np.float64))


def undecided(points, fov, w):
    """Boolean ``[M]``: an angle within ``w`` float32 steps (at the threshold) of one of the four thresholds ``fov``."""
    _, az, el = angles64(points)
    out = np.zeros(len(points), bool)
    for a, ts in ((az, fov[:2]), (el, fov[2:])):
        for t in ts:
            t = np.float32(t)
            out |= np.abs(a - np.float64(t)) <= w * np.float64(np.spacing(np.float32(abs(t))))
    return out


def scan_filter(points, words=None, lut=None, fov=None, box=None, w=1):
    """The rule on one scan.  Returns a dict: ``mask`` bool ``[M]``; ``points`` / ``labels`` (int32) / ``index`` (int32) of the kept
    rows in scan order; ``undecided`` bool ``[M]`` at width ``w`` (all False without ``fov``); ``unmapped``: whether a raw class was
    outside the map (such rows are dropped)."""
    points = np.ascontiguousarray(points, np.float32)
    M = len(points)
    mask = np.ones(M, bool)
    cls = np.zeros(M, np.int64)
    unmapped = False
    if words is not None:
        sem = (np.asarray(words).astype(np.uint32) & np.uint32(0xFFFF)).astype(np.int64)
        inside = sem < len(lut)
        cls = np.where(inside, np.asarray(lut, np.int64)[np.where(inside, sem, 0)], -1)
        unmapped = bool((cls < 0).any())
        mask &= cls > 0
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    d, az64, el64 = angles64(points)
    if box is not None:
        b = np.asarray(box, np.float64).astype(np.float32)
        with np.errstate(invalid="ignore"):
            mask &= np.logical_and.reduce((x > b[0], x < b[1], y > b[2], y < b[3], z > b[4], z < b[5], d > b[6], d < b[7]))
    und = np.zeros(M, bool)
    if fov is not None:
        t = np.asarray(fov, np.float32)
        az, el = az64.astype(np.float32), el64.astype(np.float32)
        with np.errstate(invalid="ignore"):
            mask &= (t[0] < az) & (az < t[1]) & (t[2] < el) & (el < t[3])
        und = undecided(points, t, w)
    index = np.flatnonzero(mask).astype(np.int32)
    return {"mask": mask, "points": points[mask], "labels": (cls[mask] - 1).astype(np.int32) if words is not None else None,
            "index": index, "undecided": und, "unmapped": unmapped}


def recorded_mask(raw, words, points, labels, lut):
    """The boolean mask over ``raw``'s rows that a recorded (compacted) output ``points`` / ``labels`` stands for: the recorded rows
    are a subsequence of the raw rows; they are matched in order on their bits and class."""
    cls = np.asarray(lut, np.int64)[(np.asarray(words).astype(np.uint32) & np.uint32(0xFFFF)).astype(np.int64)] - 1
    key_raw = np.concatenate([np.ascontiguousarray(raw, np.float32).view(np.uint32).astype(np.int64), cls[:, None]], 1)
    key_rec = np.concatenate([np.ascontiguousarray(points, np.float32).view(np.uint32).astype(np.int64),
                              np.asarray(labels, np.int64)[:, None]], 1)
    mask = np.zeros(len(raw), bool)
    j = 0
    for i in range(len(raw)):
        if j < len(key_rec) and (key_raw[i] == key_rec[j]).all():
            mask[i] = True
            j += 1
    assert j == len(key_rec), "the recorded rows are not a subsequence of the raw rows"
    return mask


def decided_scan(seed, M, fov=None, w=4, classes=None, lut_len=None, spread=(60.0, 60.0, 8.0)):
    """A seeded random scan ``(points [M, 4] float32, words [M] uint32)`` from which every point that is undecided at width ``w``
    has been replaced by a decided one, so the reference's float32 path and the rule give the same mask with no exceptions.
    Words carry instance bits in their upper half; ``classes``: the raw classes to draw from."""
    rng = np.random.default_rng(seed)
    fov = thresholds() if fov is None else fov

    def draw(n):
        p = rng.normal(size=(n, 4)) * np.array(spread + (0.0,)) + np.array([10.0, 0.0, 0.0, 0.0])
        p[:, 3] = rng.random(n)
        return p.astype(np.float32)
    pts = draw(M)
    for _ in range(64):
        bad = undecided(pts, fov, w)
        if not bad.any():
            break
        pts[bad] = draw(int(bad.sum()))
    assert not undecided(pts, fov, w).any()
    classes = np.arange(lut_len) if classes is None else np.asarray(classes)
    words = (classes[rng.integers(0, len(classes), M)].astype(np.uint32) | (rng.integers(0, 1 << 16, M).astype(np.uint32) << np.uint32(16)))
    return pts, words.astype(np.uint32)


def sweeps(n=4096):
    """{name: (points [n, 4] float32, the threshold's index)}: one sweep across each of the four default thresholds.  Azimuth:
    the angle stepped by 2e-8 rad at radius 10 (a float32 step at 40 deg is 6e-8 rad); elevation: z stepped by one float32 step
    at (x, y) = (10, 1), which moves the angle by about 2e-8 rad (a float32 step at 20 deg is 3e-8 rad)."""
    t = thresholds()
    out = {}
    k = np.arange(n) - n // 2
    for name, i in (("az_lo", 0), ("az_hi", 1)):
        a = np.float64(t[i]) + k * 2e-8
        out[name] = (np.stack([10 * np.cos(a), 10 * np.sin(a), np.zeros(n), np.full(n, 0.5)], 1).astype(np.float32), i)
    for name, i in (("el_lo", 2), ("el_hi", 3)):
        tan = np.tan(np.float64(t[i]))                               # el = atan2(z, d) with d the 3-D range: z = d * tan(el)
        z0 = np.float32(np.sqrt(101.0) * tan / np.sqrt(1.0 - tan * tan))
        z = z0.view(np.int32) + (k if z0 > 0 else -k).astype(np.int32)          # neighbouring floats, rising in value
        p = np.zeros((n, 4), np.float32)
        p[:, 0], p[:, 1], p[:, 2], p[:, 3] = 10.0, 1.0, z.astype(np.int32).view(np.float32), 0.5
        out[name] = (p, i)
    return out
