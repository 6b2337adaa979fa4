"""Plane RANSAC, ground removal and plane peeling (``pn2_plane_ransac`` / ``pn2_plane_refit`` / ``pn2_plane_classify``,
csrc/plane.hip; the rule is stated in include/pn2.h under "plane RANSAC" and in numpy in tests/plane_ref.py).

The reference repository has no such function: like kNN, the voxel grid, clustering, normals, ICP and the Lovasz loss this is an
extension.  It is the geometric way to name the dominant plane of a cloud, to give every row its height above the ground and to
take the ground out of a scan before ``voxel.euclidean_cluster`` -- which otherwise links cars, kerbs and poles through the road
unless a trained network says what is ground.  A fit is 3 + 2 * refine + 2 launches: hypotheses, an all-pairs scoring pass (one
hypothesis per lane, the rows broadcast from LDS), a select, ``refine`` least-squares rounds of an accumulate and a finish kernel,
and a count and a write launch that classify every row.  Nothing is read back: counts, ``min_inliers`` and the status live on the
device.  OUT OF SCOPE: MSAC / LO-RANSAC scores, an adaptive stopping rule, models other than planes, per-region ground (sloped
roads), a gradient, wiring into ``FrameSegmenter``.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib, neighbors

_p = _lib.ptr

PlaneFit = collections.namedtuple("PlaneFit", "plane count rmse dist best_h status")
PlaneSegments = collections.namedtuple("PlaneSegments", "planes counts assign status")


def workspace_bytes(N, B=1, iterations=256):
    """Bytes of the plane entry points' workspace for ``B`` clouds of up to ``N`` rows and ``iterations`` hypotheses (host-only call)."""
    return _lib.workspace_bytes("pn2_plane_workspace_bytes", (int(B), int(N), int(iterations)), ValueError,
                                "plane: B = %d clouds of N = %d rows with %d hypotheses are not supported" % (B, N, iterations))


class PlaneBuffers:
    """Everything ``fit_plane`` / ``segment_planes`` / ``ground_labels`` write, allocated once (``buffers``): ``plane`` float64 [B,4],
    ``count`` / ``best_count`` int64 [B], ``rmse`` float64 [B], ``sums`` float64 [B,10], ``dist`` float32 [B,N], ``best_h`` / ``status``
    int32 [B], ``hyp_count`` int32 [B,iterations], ``assign`` / ``labels`` int32 [B,N], ``planes`` / ``counts`` / ``statuses`` for up to
    ``max_planes`` peeled planes, the workspace, and ``error_flag`` (device int32, cleared at the start of every call; the launches OR
    ``_lib.PLANE_ERR_*`` into it)."""

    def __init__(self, N, B, iterations, device, max_planes=1):
        self.N, self.B, self.H, self.max_planes = int(N), int(B), int(iterations), int(max_planes)
        f64 = dict(device=device, dtype=torch.float64)
        i32 = dict(device=device, dtype=torch.int32)
        self.plane = torch.zeros(self.B, 4, **f64)
        self.device = self.plane.device
        self.rmse, self.sums = torch.zeros(self.B, **f64), torch.zeros(self.B, 10, **f64)
        self.count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.best_count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.best_h, self.status = torch.zeros(self.B, **i32), torch.zeros(self.B, **i32)
        self.hyp_count = torch.zeros(self.B, self.H, **i32)
        self.dist = torch.full((self.B, self.N), float("nan"), device=device, dtype=torch.float32)
        self.assign, self.labels = torch.full((self.B, self.N), -1, **i32), torch.zeros(self.B, self.N, **i32)
        self.planes = torch.zeros(self.B, self.max_planes, 4, **f64)
        self.counts = torch.zeros(self.B, self.max_planes, device=device, dtype=torch.int64)
        self.statuses = torch.zeros(self.B, self.max_planes, **i32)
        self.workspace = torch.empty(workspace_bytes(self.N, self.B, self.H), device=device, dtype=torch.uint8)
        self.error_flag = torch.zeros(1, **i32)

    def check(self, none_ok=True):
        """Reads ``error_flag`` back: ``ValueError`` for a row that takes part and is not finite and, unless ``none_ok`` (``status``
        says which clouds), for a cloud in which no plane was found."""
        flag = int(self.error_flag.item())
        if flag & _lib.PLANE_ERR_NONFINITE:
            raise ValueError("plane: a row that takes part is not finite; it was never an inlier and its distance is NaN")
        if flag & _lib.PLANE_ERR_NONE and not none_ok:
            raise ValueError("plane: a cloud has no valid hypothesis, or its best one has fewer than 3 inliers")


def buffers(N, B=1, iterations=256, device="cuda", max_planes=1):
    """Preallocates for ``B`` clouds of ``N`` rows and ``iterations`` hypotheses.  With ``buffers=`` a call allocates nothing and reads
    nothing back, and captures into a graph that stays valid when the points, the device-side counts and ``assign`` change."""
    return PlaneBuffers(N, B, iterations, device, max_planes)


def _axis(axis):
    a = np.asarray(axis, np.float64).reshape(-1)
    if a.size != 3 or not np.isfinite(a).all() or not (a != 0).any():
        raise ValueError("plane: axis must be a finite, non-zero triple")
    return (ctypes.c_double * 3)(*a)


def _cos_max(max_angle):
    if max_angle is None:
        return 0.0
    if not 0.0 <= float(max_angle) <= 90.0:
        raise ValueError("plane: max_angle is in degrees, 0 .. 90")
    return math.cos(math.radians(float(max_angle)))


def _setup(points, threshold, iterations, n_points, assign, buf, what):
    flat = isinstance(points, torch.Tensor) and points.dim() == 2
    pts = neighbors._cloud(points, what + ": points")
    B, N, _ = pts.shape
    H = int(iterations)
    if not (math.isfinite(float(threshold)) and float(threshold) >= 0.0):
        raise ValueError("%s: threshold must be finite and not negative" % what)
    if not 1 <= H <= 65536:
        raise ValueError("%s: iterations must be 1 .. 65536" % what)
    if buf is not None and (buf.B != B or buf.N != N or buf.H != H or buf.device != pts.device):
        raise ValueError("%s: the buffers were made for B = %d, N = %d, iterations = %d on %s" % (what, buf.B, buf.N, buf.H, buf.device))
    n_points = neighbors._counts(n_points, B, pts.device, what + ": n_points")
    if assign is not None:
        if not isinstance(assign, torch.Tensor) or assign.device != pts.device or assign.dtype != torch.int32 or assign.numel() != B * N or \
                not assign.is_contiguous():
            raise ValueError("%s: assign must be a contiguous int32 tensor of the points' [B, N] on their device" % what)
    return flat, pts, B, N, H, n_points


def _fit(pts, threshold, H, seed, axis, cos_max, refine, n_points, assign, plane_id, min_inliers, buf):
    """The launches of one fit on ``buf``: ransac, ``refine`` refit rounds, classify."""
    B, N, ld = pts.shape
    lib, s = _lib.load(), _lib.stream()
    buf.rmse.zero_()
    buf.count.zero_()
    _lib.check(lib.pn2_plane_ransac(_p(pts), ld, B, N, _p(n_points), _p(assign), H, int(seed) & (2 ** 64 - 1), ctypes.addressof(axis), cos_max,
                                    float(threshold), _p(buf.plane), _p(buf.hyp_count), _p(buf.best_h), _p(buf.best_count), _p(buf.status),
                                    _p(buf.error_flag), _p(buf.workspace), s), "pn2_plane_ransac")
    for _ in range(int(refine)):
        _lib.check(lib.pn2_plane_refit(_p(pts), ld, B, N, _p(n_points), _p(assign), ctypes.addressof(axis), float(threshold), _p(buf.plane),
                                       _p(buf.rmse), _p(buf.sums), _p(buf.status), _p(buf.workspace), s), "pn2_plane_refit")
    _lib.check(lib.pn2_plane_classify(_p(pts), ld, B, N, _p(n_points), _p(assign), int(plane_id), int(min_inliers), float(threshold), _p(buf.plane),
                                      _p(buf.status), _p(buf.dist), _p(buf.count), _p(buf.workspace), s), "pn2_plane_classify")


def fit_plane(points, threshold, iterations=256, seed=0, axis=(0, 0, 1), max_angle=None, refine=2, n_points=None, assign=None, plane_id=0,
              min_inliers=0, buffers=None):
    """The dominant plane of every cloud: ``iterations`` three-point hypotheses named by an integer function of ``seed``, each scored
    by its count of rows within ``threshold``, the best one (the lowest index among equals) refitted ``refine`` times by least squares
    on its inliers.

    ``points`` [N,ld] or [B,N,ld] float32 on the GPU, 3 <= ld <= 16 (a [.,4] scan is read where it lies).  The normal is turned so
    that ``n . axis >= 0``; with ``max_angle`` (degrees) a hypothesis further than that from ``axis`` is dropped: ``axis=(0, 0, 1),
    max_angle=15`` searches for the ground and cannot lock onto a wall.  ``n_points``: device int64 [B] (or host integers), only that
    many leading rows count.  ``assign``: int32 [B,N] (or [N]), read and written: only rows with ``assign < 0`` take part, and the
    inliers of the result get ``plane_id`` unless there are fewer than ``min_inliers`` of them (decided on the device).

    Returns ``PlaneFit(plane, count, rmse, dist, best_h, status)`` of device tensors: float64 [B,4] ``(n_x, n_y, n_z, d)`` with
    ``n . p + d = 0``; int64 inliers; float64 root mean square of their distances (0 with ``refine=0``); float32 [B,N] signed
    distance of EVERY row below ``n_points`` -- the height above the plane along ``axis``, NaN for a row that is not finite; the
    index of the winning hypothesis (-1: none was valid); int32 ``_lib.PLANE_NONE`` / ``PLANE_DEGENERATE`` / ``PLANE_SMALL`` bits.  A
    cloud with ``PLANE_NONE`` has a zero plane and count, and its ``dist`` and ``assign`` are not written (``dist`` keeps what the
    buffers held: NaN after allocation), as are rows at and beyond ``n_points``.  [N,ld] clouds drop the leading B."""
    what = "fit_plane"
    buf = buffers
    flat, pts, B, N, H, n_points = _setup(points, threshold, iterations, n_points, assign, buf, what)
    if int(refine) < 0 or int(plane_id) < 0:
        raise ValueError("fit_plane: refine and plane_id must not be negative")
    ax, cos_max = _axis(axis), _cos_max(max_angle)
    if buf is None:
        buf = PlaneBuffers(N, B, H, pts.device)
    else:
        buf.error_flag.zero_()
    _fit(pts, threshold, H, seed, ax, cos_max, refine, n_points, assign, plane_id, min_inliers, buf)
    res = (buf.plane, buf.count, buf.rmse, buf.dist, buf.best_h, buf.status)
    return PlaneFit(*[t[0] if flat else t for t in res])


def segment_planes(points, threshold, max_planes, min_inliers, iterations=256, seed=0, axis=(0, 0, 1), max_angle=None, refine=2, n_points=None,
                   assign=None, buffers=None):
    """``fit_plane`` run ``max_planes`` times on one ``assign`` (default: all -1): plane ``k`` is searched among the rows no earlier
    plane took, with seed ``seed + k``, and marks its inliers with ``k``.  A plane with fewer than ``min_inliers`` inliers leaves
    ``assign`` alone (``PLANE_SMALL`` in its status) -- decided on the device, nothing is read back.

    Returns ``PlaneSegments(planes, counts, assign, status)``: float64 [B,max_planes,4], int64 [B,max_planes], int32 [B,N] (-1: no
    plane), int32 [B,max_planes]; [N,ld] clouds drop the leading B."""
    what = "segment_planes"
    buf = buffers
    flat, pts, B, N, H, n_points = _setup(points, threshold, iterations, n_points, assign, buf, what)
    K = int(max_planes)
    if K < 1 or (buf is not None and buf.max_planes < K):
        raise ValueError("segment_planes: max_planes must be at least 1 and at most what the buffers were made for")
    ax, cos_max = _axis(axis), _cos_max(max_angle)
    if buf is None:
        buf = PlaneBuffers(N, B, H, pts.device, K)
    else:
        buf.error_flag.zero_()
    if assign is None:
        assign = buf.assign
        assign.fill_(-1)
    for k in range(K):
        _fit(pts, threshold, H, int(seed) + k, ax, cos_max, refine, n_points, assign, k, min_inliers, buf)
        buf.planes[:, k].copy_(buf.plane)
        buf.counts[:, k].copy_(buf.count)
        buf.statuses[:, k].copy_(buf.status)
    assign = assign.view(B, N)
    res = (buf.planes[:, :K], buf.counts[:, :K], assign, buf.statuses[:, :K])
    return PlaneSegments(*[t[0] if flat else t for t in res])


def ground_labels(points, threshold=0.2, max_angle=15.0, iterations=256, seed=0, axis=(0, 0, 1), refine=2, n_points=None, buffers=None):
    """int32 labels [B,N] (or [N]): -1 on the ground -- the inliers of ``fit_plane(points, threshold, axis=axis, max_angle=max_angle)``
    -- and 0 elsewhere: exactly what ``voxel.euclidean_cluster(points, labels=...)`` takes, since a voxel with a negative label takes
    no part.  Ground removal plus clustering is two calls and needs no network.  The fit itself is left in ``buffers``."""
    what = "ground_labels"
    buf = buffers
    flat, pts, B, N, H, n_points = _setup(points, threshold, iterations, n_points, None, buf, what)
    ax, cos_max = _axis(axis), _cos_max(max_angle)
    if buf is None:
        buf = PlaneBuffers(N, B, H, pts.device)
    else:
        buf.error_flag.zero_()
    buf.assign.fill_(-1)
    _fit(pts, threshold, H, seed, ax, cos_max, refine, n_points, buf.assign, 0, 0, buf)
    torch.neg(buf.assign, out=buf.labels)                          # inliers 0 -> -1, the rest -1 -> 0
    buf.labels.sub_(1)
    return buf.labels[0] if flat else buf.labels


def height_above(points, plane):
    """``(n . p) + d`` for every row of ``points`` [N,ld] or [B,N,ld] float32 against ``plane`` [4] or [B,4] -- ``((n_x x + n_y y) + n_z z)
    + d`` in float64, each operation rounded on its own, rounded once to float32: ``fit_plane``'s ``dist`` for any plane.  Plain torch."""
    flat = points.dim() == 2
    p = (points[None] if flat else points)[:, :, :3].to(torch.float64)
    P = plane.to(device=p.device, dtype=torch.float64).reshape(-1, 4)[:, :, None]
    r = ((P[:, 0] * p[:, :, 0] + P[:, 1] * p[:, :, 1]) + P[:, 2] * p[:, :, 2]) + P[:, 3]
    r = r.to(torch.float32)
    return r[0] if flat else r
