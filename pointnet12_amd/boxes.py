"""Oriented bounding boxes per segment (``pn2_segment_boxes``, csrc/boxes.hip): where an instance is, how big it is and which way
it points -- the length, width, height and heading box every consumer of a clustering asks for first.

For every segment of an ``inverse``-style map (``VoxelGrid.components`` / ``euclidean_cluster``'s ``row_component`` and ``count``, or
any other) and every angle of a table over [0, pi/2) the rows are projected on the angle's axes; the angle whose rectangle has the most
rows CLOSE TO ITS EDGES wins (the closeness criterion of Zhang et al., IV 2017, quantised to integers), the smaller area among equals,
the lowest angle after that.  The criterion is not the minimum-area rectangle on purpose: a car seen from a corner is an L, the hull of
an L is a right triangle, and a right triangle's rectangle flush with a leg and the one flush with the hypotenuse have EXACTLY the same
area -- noise decides (tests/test_boxes_cpu.py: a median yaw error above 10 degrees against a third of a degree).  Every output is an
integer, a minimum or a maximum, so the result is byte-identical from run to run and under any permutation of the rows.  The rule is
stated in include/pn2.h under "segment boxes" and, in numpy, in tests/box_ref.py.

``canonical`` / ``corners`` / ``contains`` are plain torch on the small per-segment tensors.

Out of scope: 3-D orientation (pitch / roll), convex hulls and the exact rotating-calipers rectangle, the variance criterion, angle
refinement below the table step, box IoU / NMS, tracking, a gradient, and drawing boxes into the demo images.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from .voxel import _segment_args

Boxes = collections.namedtuple("Boxes", "center size yaw angle lo hi n score")
Boxes.__doc__ = """What ``segment_boxes`` returns, device tensors with one row per segment (segment s of cloud b at ``out_begin[b] + s``):
``center`` float32 ``[S, 3]`` (in the points' own axes order: ground plane x, y, then height), ``size`` float32 ``[S, 3]`` (the extent
along the heading, across it, and the height), ``yaw`` float32 ``[S]`` in [0, pi/2) (the heading is known up to a quarter turn:
``canonical`` puts the longer side first), ``angle`` int32 (the table index, -1 for a segment without rows), ``lo`` / ``hi`` float32
``[S, 3]`` (the axis-aligned box), ``n`` int32 (the rows that took part) and ``score`` int64 (the winning angle's closeness score)."""


def angle_table(angles=64, device="cuda"):
    """The table ``pn2_segment_boxes`` reads: float32 ``[A, 4]`` of ``(cos, sin, theta, 0)`` for ``theta_a = a * (pi / 2) / A``, computed in
    fp64 and rounded once.  ``angles``: A, 1 .. 256."""
    return torch.from_numpy(angle_table_np(angles)).to(device)


def angle_table_np(angles=64):
    A = int(angles)
    if not 1 <= A <= _lib.BOX_MAX_ANGLES:
        raise ValueError("boxes: 1 <= angles <= %d" % _lib.BOX_MAX_ANGLES)
    theta = np.arange(A, dtype=np.float64) * (math.pi / 2) / A
    table = np.zeros((A, 4), np.float32)
    table[:, 0], table[:, 1], table[:, 2] = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32), theta.astype(np.float32)
    return table


class BoxBuffers:
    """The static buffers of one ``segment_boxes`` call shape (``boxes.buffers``): the eight outputs for ``rows`` segments, the kernel's
    ``workspace`` for ``B`` clouds of at most ``max_rows`` rows, the angle ``table`` and ``error_flag`` (device int32, cleared by every call
    that is given these buffers; ``check()`` reads it back).  Rows no call writes hold zeros (``angle``: -1)."""

    def __init__(self, rows, B, max_rows, angles, device):
        nbytes = _lib.workspace_bytes("pn2_segment_boxes_workspace_bytes", (int(B), int(max_rows)), _lib.Pn2Error,
                                      "BoxBuffers: B = %d, max_rows = %d are not supported" % (B, max_rows))
        self.rows, self.B, self.max_rows, self.angles = int(rows), int(B), int(max_rows), int(angles)
        f = lambda *shape: torch.zeros(*shape, device=device, dtype=torch.float32)
        self.center, self.size, self.lo, self.hi, self.yaw = f(self.rows, 3), f(self.rows, 3), f(self.rows, 3), f(self.rows, 3), f(self.rows)
        self.angle = torch.full((self.rows,), -1, device=device, dtype=torch.int32)
        self.n = torch.zeros(self.rows, device=device, dtype=torch.int32)
        self.score = torch.zeros(self.rows, device=device, dtype=torch.int64)
        self.workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)
        self.table = angle_table(self.angles, device)
        self.error_flag = torch.zeros(1, device=device, dtype=torch.int32)

    def boxes(self):
        return Boxes(self.center, self.size, self.yaw, self.angle, self.lo, self.hi, self.n, self.score)

    def check(self):
        """Reads ``error_flag`` back: ``ValueError`` for a row that names a segment at or beyond the count, or for a row of a segment
        that is not finite (or beyond 2**60 in the ground plane) and was left out of its box."""
        check_flag(int(self.error_flag.item()))


def check_flag(flag):
    if flag & _lib.BOX_ERR_RANGE:
        raise ValueError("segment_boxes: a row names a segment at or beyond the segment count")
    if flag & _lib.BOX_ERR_NONFINITE:
        raise ValueError("segment_boxes: a row of a segment is not finite (or beyond 2**60 in the ground plane); it was left out of its box")


def buffers(rows, B=1, max_rows=None, angles=64, device="cuda"):
    """``BoxBuffers`` for ``segment_boxes`` calls of ``B`` clouds of at most ``max_rows`` rows each (default ``rows``) whose segments fit
    ``rows`` output rows, with a table of ``angles`` angles."""
    return BoxBuffers(rows, B, rows if max_rows is None else max_rows, angles, torch.device(device))


def segment_boxes(points, inverse, count, angles=64, d0=0.05, criterion="closeness", axes=(0, 1, 2), n_points=None, row_begin=None,
                  row_count=None, max_rows=None, out_begin=None, out_rows=None, buffers=None, split_rows=0, error_flag=None):
    """One oriented box per segment, as ``Boxes`` of device tensors (``pn2_segment_boxes``; the rule of include/pn2.h).

    ``points``: float32 ``[rows, ld]`` on the device, read where it lies (a ``[rows, 4]`` scan with its remission is fine); ``axes``:
    the columns of the two ground-plane coordinates and of the height (KITTI's z-up: ``(0, 1, 2)``).  ``inverse``: int32 ``[rows]``, the
    segment (rank inside its cloud) of every row, negative = the row takes no part; ``count``: the number of segments, an int or an
    int64 ``[B]`` DEVICE tensor.  One cloud, or B clouds with ``row_begin`` / ``row_count`` / ``max_rows`` / ``out_begin`` exactly as
    ``voxel.segment_mean`` takes them; ``out_rows``: the rows of the result (default ``rows``).  ``n_points`` is accepted for symmetry
    with ``segment_mean`` and not used: rows that are not finite take no part, so the rows are always counted here (``Boxes.n``).

    ``angles``: the table's length A (headings ``a * 90 / A`` degrees), ``d0``: the closeness criterion's distance floor in the points'
    unit (5 cm), ``criterion``: ``"closeness"``, or ``"area"`` for the minimum-area rectangle over the table (``d0 = 0``; the tie-break
    of the default, and what the module's docstring warns about).  ``split_rows``: the rows from which a segment is swept by a
    workgroup instead of a wave (0: the library's 4096); the bytes do not depend on it.

    Segments without rows give zeros and ``angle`` -1; rows of the result at or beyond the count are not written (zeros / -1 in
    tensors made here).  With ``buffers`` (``boxes.buffers``: outputs, workspace, table, ``error_flag``) and device-side counts the call
    allocates nothing, reads nothing back and can be captured in a graph that stays valid when the points, ``inverse`` and the
    counts change; ``buffers.check()`` raises for the two error bits.  ``error_flag`` (device int32 ``[1]``): the word that collects
    the bits INSTEAD of the buffers' own; it is not cleared here, so one word can serve a downsample -> cluster -> boxes chain.
    Without ``buffers`` and ``error_flag`` the error bits are dropped."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _lib.Pn2Error("segment_boxes: points must live on the GPU: this package has no CPU path")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3 or not points.is_contiguous():
        raise ValueError("segment_boxes: points must be a contiguous float32 [rows, ld] tensor, ld >= 3")
    if criterion not in ("closeness", "area"):
        raise ValueError('segment_boxes: criterion is "closeness" or "area"')
    rows, ld, dev = int(points.shape[0]), int(points.shape[1]), points.device
    cx, cy, cz = (int(a) for a in axes)
    if len({cx, cy, cz}) != 3 or min(cx, cy, cz) < 0 or max(cx, cy, cz) >= ld:
        raise ValueError("segment_boxes: axes are three distinct columns below %d" % ld)
    d0 = 0.0 if criterion == "area" else float(d0)
    if not math.isfinite(d0):
        raise ValueError("segment_boxes: d0 must be finite")
    inverse, count, row_begin, row_count, B, max_rows, out_begin = _segment_args("segment_boxes", rows, inverse, count, row_begin, row_count,
                                                                                max_rows, out_begin, dev)
    out_rows = rows if out_rows is None else int(out_rows)
    if error_flag is not None and (not error_flag.is_cuda or error_flag.dtype != torch.int32 or error_flag.numel() != 1):
        raise ValueError("segment_boxes: error_flag must be a device int32 tensor of one element")
    err = error_flag
    if buffers is None:
        buffers = BoxBuffers(out_rows, B, max_rows, angles, dev)
    else:
        if buffers.B != B or buffers.max_rows < max_rows or buffers.rows < out_rows or buffers.angles != int(angles):
            raise ValueError("segment_boxes: buffers were made for B = %d, max_rows = %d, %d rows, %d angles"
                             % (buffers.B, buffers.max_rows, buffers.rows, buffers.angles))
        if err is None:
            buffers.error_flag.zero_()                               # an async fill, nothing is read back
            err = buffers.error_flag
    p, b = _lib.ptr, buffers
    # (max_rows as the buffers were made for: the workspace layout follows it)
    _lib.check(_lib.load().pn2_segment_boxes(p(points), ld, cx, cy, cz, p(inverse), p(row_begin), p(row_count), B, b.max_rows, p(out_begin),
                                             p(count), p(b.table), b.angles, d0, int(split_rows), p(b.center), p(b.size), p(b.yaw), p(b.angle),
                                             p(b.lo), p(b.hi), p(b.n), p(b.score), p(err), p(b.workspace), _lib.stream()),
               "pn2_segment_boxes")
    return b.boxes()


def instance_boxes(points, clusters, **kw):
    """``segment_boxes(points, clusters.row_component, clusters.count, ...)`` on the ``Components`` that ``VoxelGrid.components`` /
    ``euclidean_cluster`` return: one box per instance, at ``out_begin[b] + id``."""
    return segment_boxes(points, clusters.row_component, clusters.count, **kw)


def canonical(boxes):
    """The same boxes with the LONGER ground-plane side first: where ``size[:, 0] < size[:, 1]`` the two are swapped and the yaw gains
    pi / 2, so yaw lies in [0, pi).  ``center``, ``angle``, ``lo``, ``hi``, ``n``, ``score`` are unchanged."""
    swap = boxes.size[:, 0] < boxes.size[:, 1]
    size = torch.where(swap[:, None], boxes.size[:, [1, 0, 2]], boxes.size)
    yaw = torch.where(swap, boxes.yaw + math.pi / 2, boxes.yaw)
    return boxes._replace(size=size, yaw=yaw)


def corners(boxes):
    """The eight corners, float32 ``[S, 8, 3]``: corner k = ``center + R(yaw) @ (sx * l / 2, sy * w / 2) , z +- h / 2`` with the signs
    ``(sx, sy, sz)`` = ((k & 1), (k >> 1) & 1, (k >> 2) & 1) mapped 0 -> -1, 1 -> +1: the bottom face first, then the top."""
    k = torch.arange(8, device=boxes.center.device)
    sign = torch.stack([(k & 1), (k >> 1) & 1, (k >> 2) & 1], 1).to(boxes.center.dtype) * 2 - 1       # [8, 3]
    half = boxes.size[:, None, :] * 0.5 * sign[None]                                                      # [S, 8, 3]
    c, s = torch.cos(boxes.yaw)[:, None], torch.sin(boxes.yaw)[:, None]
    x = c * half[..., 0] - s * half[..., 1]
    y = s * half[..., 0] + c * half[..., 1]
    return boxes.center[:, None, :] + torch.stack([x, y, half[..., 2]], -1)


def contains(boxes, points, row_component, axes=(0, 1, 2), margin=0.0):
    """bool per row: does row i lie inside the box of ITS segment ``row_component[i]`` (one cloud; False for a negative id), up to
    ``margin`` on every side?  ``points``: ``[rows, ld]``, ``axes`` as ``segment_boxes`` took them."""
    ids = row_component.long()
    at = ids.clamp(min=0)
    centre, size, yaw = boxes.center[at], boxes.size[at], boxes.yaw[at]
    dx, dy, dz = (points[:, a] - centre[:, i] for i, a in enumerate(axes))
    c, s = torch.cos(yaw), torch.sin(yaw)
    u, v = c * dx + s * dy, c * dy - s * dx
    half = size * 0.5 + margin
    return (ids >= 0) & (u.abs() <= half[:, 0]) & (v.abs() <= half[:, 1]) & (dz.abs() <= half[:, 2])
