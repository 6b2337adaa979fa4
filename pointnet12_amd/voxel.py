"""Voxel-grid downsampling on the device (``pn2_voxel_grid``, csrc/voxel.hip): one row per occupied cell of a regular grid.

The grid subsample of every LiDAR code base: of the rows that fall into one cell the one with the lowest row number is kept, the
kept rows stay in the cloud's order (a stable compaction, ``np.sort(np.unique(key, return_index=True)[1])``), and every input
row learns which output row stands for it (``inverse``).  The kept COUNT stays in device memory, where ``pn2_prepare_clouds`` and
the device-side choice read it; nothing is read back or allocated by a call with ``out=``, so it captures into a graph, and the
result is byte-identical from run to run.  The rule is stated in include/pn2.h (and, in numpy, in tests/voxel_ref.py).

``VoxelGrid(reduce="mean", label_reduce="mode")`` returns the voxel's MEAN row (centroid and mean remission) and its MAJORITY label
instead of the lowest row's: order-free integer segment reductions over ``inverse`` (``pn2_segment_mean`` / ``pn2_segment_mode``,
csrc/voxel_reduce.hip; the rules are in include/pn2.h and, in numpy, in tests/voxel_reduce_ref.py), byte-identical from run to run
like everything else here.  ``segment_mean`` / ``segment_mode`` run them over any ``inverse``-style map, ``pool_mean`` is the mean as
an autograd function.

``VoxelGrid.components`` / ``euclidean_cluster`` give every voxel and every row an INSTANCE id: Euclidean clustering, the connected
components of the occupied cells under 6 / 18 / 26 connectivity, optionally per label and per class set (``pn2_voxel_components``,
csrc/voxel_cluster.hip; the rule is in include/pn2.h and, in numpy, in tests/cluster_ref.py).  The ids are numbered by the
components' lowest row, the count stays on the device and ``row_component`` is an ``inverse``-style map again:
``segment_mean(points, row_component, count)`` gives the instances' centroids.

Out of scope: a search radius beyond the 26 neighbouring cells, clustering without a grid (DBSCAN with a density test), ids tracked
across frames, more than 16 columns per reduction, per-column max / min pooling and grids over more than three key columns.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib


def _triple(v, what):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError("VoxelGrid: %s must be a scalar or a triple" % what)
    return np.ascontiguousarray(a)


class VoxelBuffers:
    """The static buffers of one ``VoxelGrid.downsample`` call shape (``VoxelGrid.buffers``): ``points`` float32 ``[rows, ld]``,
    ``labels`` / ``index`` / ``inverse`` / ``n_points`` int32 ``[rows]``, ``count`` int64 ``[B]`` and the kernel's ``workspace``.
    ``reduce=True`` (what a grid with ``reduce="mean"`` or ``label_reduce="mode"`` asks for) adds ``reduce_workspace``, the segment
    reductions' workspace, and ``votes`` int32 ``[rows]``; both are None otherwise."""

    def __init__(self, rows, B, max_rows, ld, device, reduce=False):
        nbytes = _lib.workspace_bytes("pn2_voxel_grid_workspace_bytes", (int(B), int(max_rows)), _lib.Pn2Error,
                                      "VoxelBuffers: B = %d, max_rows = %d are not supported" % (B, max_rows))
        self.rows, self.B, self.max_rows, self.ld = int(rows), int(B), int(max_rows), int(ld)
        i32 = lambda: torch.empty(self.rows, device=device, dtype=torch.int32)
        self.points = torch.empty(self.rows, self.ld, device=device, dtype=torch.float32)
        self.labels, self.index, self.inverse, self.n_points = i32(), i32(), i32(), i32()
        self.count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)
        self.reduce_workspace = self.votes = None
        if reduce:
            nbytes = _lib.workspace_bytes("pn2_segment_reduce_workspace_bytes", (self.B, self.max_rows, self.ld), _lib.Pn2Error,
                                          "VoxelBuffers: B = %d, max_rows = %d, ld = %d are not supported" % (B, max_rows, ld))
            self.reduce_workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)
            self.votes = i32()


Components = collections.namedtuple("Components", "row_component voxel_component count root n_points n_voxels label")
Components.__doc__ = """What ``VoxelGrid.components`` returns, all device tensors: ``row_component`` int32 per row and ``voxel_component``
int32 per voxel (the id inside the cloud, -1 for none), ``count`` int64 ``[B]``, and per component at ``comp_begin[b] + id``: ``root`` (the
rank of its lowest voxel), ``n_points``, ``n_voxels`` and ``label`` (int32)."""


class ComponentBuffers:
    """The static buffers of one ``VoxelGrid.components`` call shape (``VoxelGrid.component_buffers``): ``row_component`` /
    ``voxel_component`` / ``root`` / ``n_points`` / ``n_voxels`` / ``label`` int32 ``[rows]``, ``count`` int64 ``[B]`` and the kernel's
    ``workspace``."""

    def __init__(self, rows, B, max_rows, device):
        nbytes = _lib.workspace_bytes("pn2_voxel_components_workspace_bytes", (int(B), int(max_rows)), _lib.Pn2Error,
                                      "ComponentBuffers: B = %d, max_rows = %d are not supported" % (B, max_rows))
        self.rows, self.B, self.max_rows = int(rows), int(B), int(max_rows)
        i32 = lambda: torch.full((self.rows,), -1, device=device, dtype=torch.int32)
        self.row_component, self.voxel_component = i32(), i32()
        self.root, self.n_points, self.n_voxels, self.label = i32(), i32(), i32(), i32()
        self.count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)


class VoxelGrid:
    """A regular grid of cells ``voxel_size`` wide (a scalar or one size per axis) whose cell 0 starts at ``origin`` (likewise):
    a point p lies in cell ``floor((float64(p) - origin) / voxel_size)`` per axis, and cells from -2**20 to 2**20 - 1 exist.

    ``error_flag`` (device int32, cleared at the start of every ``downsample``) collects ``_lib.VOXEL_ERR_RANGE`` (a row with a
    non-finite coordinate or outside the grid: it is dropped and its ``inverse`` is -1) and ``_lib.VOXEL_ERR_ROWS`` (a
    ``row_count`` above ``max_rows``: the rows beyond are ignored); ``check()`` reads it back and raises ``ValueError``.

    ``reduce``: what ``downsample`` returns as a voxel's ``points`` row -- ``"first"``: its lowest row, bit for bit; ``"mean"``: the
    mean of ALL ``ld`` columns over the voxel's rows (the centroid plus mean remission; ``pn2_segment_mean``'s rule, include/pn2.h).
    ``label_reduce``: its label -- ``"first"``: the lowest row's; ``"mode"``: the majority label of the voxel's rows with a label
    >= 0, the lowest label among equals, -1 without one (``pn2_segment_mode``; the winner's count is left in the buffers'
    ``votes``).  ``index`` / ``count`` / ``inverse`` / ``n_points`` do not depend on either.  The reductions add
    ``_lib.SEGMENT_ERR_NONFINITE`` to ``error_flag`` (a NaN / inf in a column that is no coordinate: that voxel's mean of that column is
    NaN) and ``_lib.SEGMENT_ERR_RANGE`` (cannot happen with the grid's own ``inverse``); ``components`` adds ``_lib.CLUSTER_ERR_*``
    (none can happen with the grid's own ``downsample`` result and counts within ``max_rows``)."""

    def __init__(self, voxel_size, origin=0.0, device="cuda", reduce="first", label_reduce="first"):
        if reduce not in ("first", "mean") or label_reduce not in ("first", "mode"):
            raise ValueError('VoxelGrid: reduce is "first" or "mean", label_reduce "first" or "mode"')
        self.reduce, self.label_reduce = reduce, label_reduce
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Pn2Error("VoxelGrid: the HIP device is the only implementation")
        self.voxel_size, self.origin = _triple(voxel_size, "voxel_size"), _triple(origin, "origin")
        if not (np.isfinite(self.voxel_size).all() and (self.voxel_size > 0).all() and np.isfinite(self.origin).all()):
            raise ValueError("VoxelGrid: voxel_size must be finite and > 0, origin finite")
        self.error_flag = torch.zeros(1, device=self.device, dtype=torch.int32)

    def buffers(self, rows, B=1, max_rows=None, ld=4):
        """``VoxelBuffers`` for calls of ``B`` clouds of at most ``max_rows`` rows each (default ``rows``) whose inputs and outputs
        fit ``rows`` rows of ``ld`` floats."""
        return VoxelBuffers(rows, B, rows if max_rows is None else max_rows, ld, self.device, self.reduces)

    @property
    def reduces(self):
        """Whether ``downsample`` runs a segment reduction (its buffers then carry ``reduce_workspace``)."""
        return self.reduce == "mean" or self.label_reduce == "mode"

    def _regular_rows(self, points):
        """``row_begin`` / ``row_count`` of ``[M, ld]`` (one cloud) or ``[B, M, ld]`` points (kept: a second call of the same shape
        allocates nothing)."""
        M = int(points.shape[-2])
        held = getattr(self, "_regular", None)
        if held is None or held[0] != (points.dim(), int(points.shape[0]), M):
            nb = 1 if points.dim() == 2 else int(points.shape[0])
            held = self._regular = ((points.dim(), int(points.shape[0]), M),
                                    torch.arange(nb, device=self.device, dtype=torch.int64) * M,
                                    torch.full((nb,), M, device=self.device, dtype=torch.int64))
        return held[1], held[2]

    def downsample(self, points, labels=None, row_begin=None, row_count=None, max_rows=None, out=None, out_begin=None):
        """``(points, labels, index, count, inverse, n_points)`` as device tensors.  ``points``: float32 on the device, ``[M, ld]``
        (one cloud, or B clouds back to back with ``row_begin`` / ``row_count``: int64 ``[B]`` DEVICE tensors as
        ``pn2_prepare_clouds`` reads them) or ``[B, M, ld]`` contiguous (``row_begin`` = b * M and ``row_count`` = M unless
        given), 3 <= ld <= 16, columns 0..2 = x, y, z.  ``labels``: int32 ``[rows]`` or None (``labels`` of the result is then None).
        ``max_rows``: a host bound of every count (None: M).

        Cloud b's voxels are rows ``out_begin[b] : out_begin[b] + count[b]`` of the outputs (``out_begin``: int64 ``[B]`` on the
        device, None: ``row_begin``), in the order of their representatives -- each voxel's lowest row: ``points`` (that row, all
        ``ld`` floats bit for bit; with ``reduce="mean"`` the mean of the voxel's rows), ``labels`` (its label; with
        ``label_reduce="mode"`` the voxel's majority label), ``index`` int32 (its row inside the cloud, strictly increasing) and
        ``n_points`` int32 (the valid rows in the voxel); rows outside those ranges are not written.  ``inverse`` int32 ``[rows]``:
        for row ``row_begin[b] + i`` the rank of its voxel inside cloud b (-1: the row was dropped).  ``count`` is int64 ``[B]`` and
        stays on the device.  With ``out`` (a ``VoxelBuffers`` of this shape) and ``row_begin`` / ``row_count`` given (or the
        ``[B, M, ld]`` form, B = 1 included) the call allocates nothing and can be captured in a graph; a captured call stays valid
        when ``row_count``'s content changes."""
        if not isinstance(points, torch.Tensor) or not points.is_cuda:
            raise _lib.Pn2Error("VoxelGrid.downsample: points must live on the GPU: this package has no CPU path")
        if points.dtype != torch.float32 or points.dim() not in (2, 3) or not 3 <= points.shape[-1] <= 16 or not points.is_contiguous():
            raise ValueError("VoxelGrid.downsample: points must be a contiguous float32 [M, ld] or [B, M, ld] tensor, 3 <= ld <= 16")
        ld, M = int(points.shape[-1]), int(points.shape[-2])
        rows = M if points.dim() == 2 else int(points.shape[0]) * M
        if labels is not None and (not labels.is_cuda or labels.dtype != torch.int32 or labels.numel() != rows or not labels.is_contiguous()):
            raise ValueError("VoxelGrid.downsample: labels must be a contiguous int32 device tensor, one per row")
        if (row_begin is None) != (row_count is None):
            raise ValueError("VoxelGrid.downsample: row_begin and row_count go together")
        if row_begin is None:
            row_begin, row_count = self._regular_rows(points)
        B = int(row_begin.numel())
        for t in (row_begin, row_count) + (() if out_begin is None else (out_begin,)):
            if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
                raise ValueError("VoxelGrid.downsample: row_begin, row_count and out_begin must be int64 [B] device tensors")
        max_rows = M if max_rows is None else int(max_rows)
        if out is None:
            out = VoxelBuffers(rows, B, max_rows, ld, self.device, self.reduces)
        elif out.B != B or out.max_rows < max_rows or out.ld != ld or out.rows < rows:
            raise ValueError("VoxelGrid.downsample: out was made for B = %d, max_rows = %d, ld = %d, %d rows"
                             % (out.B, out.max_rows, out.ld, out.rows))
        mean, mode = self.reduce == "mean", self.label_reduce == "mode" and labels is not None
        if (mean or mode) and out.reduce_workspace is None:
            raise ValueError("VoxelGrid.downsample: out was made without the reductions' workspace (VoxelGrid.buffers of THIS grid has it)")
        p = _lib.ptr
        dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ob = row_begin if out_begin is None else out_begin
        self.error_flag.zero_()                                      # an async fill, nothing is read back
        # (max_rows as the buffers were made for: the workspace layout follows it)
        _lib.check(_lib.load().pn2_voxel_grid(p(points), ld, p(labels), p(row_begin), p(row_count), B, out.max_rows, dp(self.origin),
                                              dp(self.voxel_size), p(ob), None if mean else p(out.points),
                                              p(out.labels) if labels is not None and not mode else None, p(out.index), p(out.count),
                                              p(out.inverse), p(out.n_points), p(self.error_flag), p(out.workspace), _lib.stream()),
                   "pn2_voxel_grid")
        # the reductions read `inverse`, `count` and `n_points` where the launches above left them: device memory, nothing read back
        if mean:
            _lib.check(_lib.load().pn2_segment_mean(p(points), ld, ld, p(out.inverse), p(row_begin), p(row_count), B, out.max_rows, p(ob),
                                                    p(out.count), p(out.n_points), p(out.points), ld, None, p(self.error_flag),
                                                    p(out.reduce_workspace), _lib.stream()), "pn2_segment_mean")
        if mode:
            _lib.check(_lib.load().pn2_segment_mode(p(labels), p(out.inverse), p(row_begin), p(row_count), B, out.max_rows, p(ob),
                                                    p(out.count), -1, p(out.labels), p(out.votes), p(self.error_flag),
                                                    p(out.reduce_workspace), _lib.stream()), "pn2_segment_mode")
        return out.points, (out.labels if labels is not None else None), out.index, out.count, out.inverse, out.n_points

    def component_buffers(self, rows, B=1, max_rows=None):
        """``ComponentBuffers`` for ``components`` calls of ``B`` clouds of at most ``max_rows`` rows each (default ``rows``) whose
        rows, voxels and components fit ``rows`` entries."""
        return ComponentBuffers(rows, B, rows if max_rows is None else max_rows, self.device)

    def components(self, points, down, row_labels=None, connectivity=26, same_label=True, member=None, min_points=1, min_voxels=1,
                   row_begin=None, row_count=None, max_rows=None, out_begin=None, comp_begin=None, out=None):
        """Euclidean clustering of a ``downsample`` result (``pn2_voxel_components``; the rule of include/pn2.h): the connected
        components of the occupied cells, as ``Components`` of device tensors.

        ``points``, ``row_begin`` / ``row_count`` / ``max_rows`` / ``out_begin``: what ``downsample`` was called with; ``down``: what it
        returned (its ``labels``, if any, are the voxels' labels).  Two voxels of one cloud are adjacent iff both TAKE PART and their
        cells differ by at most 1 on every axis, in at most 1 / 2 / 3 axes for ``connectivity`` 6 / 18 / 26, and -- with
        ``same_label`` and labelled voxels -- carry the same label.  A labelled voxel takes part iff its label is >= 0 and, with
        ``member`` (int32 ``[L]`` on the device, or a host sequence of L flags that is uploaded here), ``member[label] != 0``; a label
        at or beyond L takes no part.  A component is kept iff it has at least ``min_points`` rows and ``min_voxels`` voxels; the kept
        ones get ids 0 .. ``count[b]`` - 1 in ascending order of their lowest voxel (= lowest row).

        ``voxel_component`` (int32 at ``out_begin[b] + v``): the id, -1 for a voxel that takes no part or whose component is not kept.
        ``row_component`` (int32 per row): its voxel's id, -1 for a row the grid dropped and, with ``row_labels`` (int32 per row;
        needs labelled voxels), for a row whose label differs from its voxel's.  It is an ``inverse``-style map:
        ``segment_mean(points, row_component, count)`` gives the centroids, ``segment_mode`` the majority class.  ``root`` /
        ``n_points`` / ``n_voxels`` / ``label`` (int32 at ``comp_begin[b] + id``; ``comp_begin``: int64 ``[B]`` on the device, None:
        ``out_begin``): the component's lowest voxel rank, its rows, its voxels and its root's label (0 without labels).  ``count`` is
        int64 ``[B]`` and stays on the device.  Entries outside those ranges are not written (-1 in buffers made here).

        With ``out`` (``component_buffers``), device-side ``member`` and ``row_begin`` / ``row_count`` given (or the ``[B, M, ld]``
        form) the call allocates nothing, reads nothing back and can be captured in a graph that stays valid when the counts
        change.  ``error_flag`` is NOT cleared here: it goes on collecting after ``downsample``.  Byte-identical from run to run."""
        if not isinstance(points, torch.Tensor) or not points.is_cuda:
            raise _lib.Pn2Error("VoxelGrid.components: points must live on the GPU: this package has no CPU path")
        if points.dtype != torch.float32 or points.dim() not in (2, 3) or not 3 <= points.shape[-1] <= 16 or not points.is_contiguous():
            raise ValueError("VoxelGrid.components: points must be a contiguous float32 [M, ld] or [B, M, ld] tensor, 3 <= ld <= 16")
        if connectivity not in (6, 18, 26):
            raise ValueError("VoxelGrid.components: connectivity is 6, 18 or 26")
        if int(min_points) < 1 or int(min_voxels) < 1:
            raise ValueError("VoxelGrid.components: min_points and min_voxels are at least 1")
        ld, M = int(points.shape[-1]), int(points.shape[-2])
        rows = M if points.dim() == 2 else int(points.shape[0]) * M
        _, vox_labels, index, count, inverse, n_points = down
        if (row_begin is None) != (row_count is None):
            raise ValueError("VoxelGrid.components: row_begin and row_count go together")
        if row_begin is None:
            row_begin, row_count = self._regular_rows(points)
        B = int(row_begin.numel())
        out_begin = row_begin if out_begin is None else out_begin
        comp_begin = out_begin if comp_begin is None else comp_begin
        for t in (row_begin, row_count, out_begin, comp_begin, count):
            if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
                raise ValueError("VoxelGrid.components: row_begin, row_count, out_begin, comp_begin and the voxel count must be "
                                 "int64 [B] device tensors")
        for name, t, need in (("index", index, True), ("inverse", inverse, True), ("n_points", n_points, True),
                              ("the voxels' labels", vox_labels, False), ("row_labels", row_labels, False)):
            if t is None and not need:
                continue
            if t is None or not t.is_cuda or t.dtype != torch.int32 or t.numel() < rows or not t.is_contiguous():
                raise ValueError("VoxelGrid.components: %s must be a contiguous int32 device tensor of at least %d entries" % (name, rows))
        if vox_labels is None and (row_labels is not None or member is not None):
            raise ValueError("VoxelGrid.components: row_labels and member need labelled voxels (downsample with labels)")
        if member is not None and not isinstance(member, torch.Tensor):
            member = torch.tensor([1 if m else 0 for m in member], device=self.device, dtype=torch.int32)
        if member is not None and (not member.is_cuda or member.dtype != torch.int32 or member.dim() != 1 or member.numel() < 1 or
                                   not member.is_contiguous()):
            raise ValueError("VoxelGrid.components: member must be a contiguous int32 [L] device tensor")
        max_rows = M if max_rows is None else int(max_rows)
        if out is None:
            out = ComponentBuffers(rows, B, max_rows, self.device)
        elif out.B != B or out.max_rows < max_rows or out.rows < rows:
            raise ValueError("VoxelGrid.components: out was made for B = %d, max_rows = %d, %d rows" % (out.B, out.max_rows, out.rows))
        p = _lib.ptr
        dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        # (max_rows as the buffers were made for: the workspace layout follows it)
        _lib.check(_lib.load().pn2_voxel_components(p(points), ld, p(row_begin), p(row_count), B, out.max_rows, dp(self.origin),
                                                    dp(self.voxel_size), p(out_begin), p(count), p(index), p(n_points), p(vox_labels),
                                                    p(inverse), p(row_labels), int(connectivity), 1 if same_label else 0, p(member),
                                                    0 if member is None else int(member.numel()), int(min_points), int(min_voxels),
                                                    p(comp_begin), p(out.voxel_component), p(out.row_component), p(out.root),
                                                    p(out.n_points), p(out.n_voxels), p(out.label), p(out.count), p(self.error_flag),
                                                    p(out.workspace), _lib.stream()), "pn2_voxel_components")
        return Components(out.row_component, out.voxel_component, out.count, out.root, out.n_points, out.n_voxels, out.label)

    def check(self):
        """Reads ``error_flag`` back: ``ValueError`` for a row outside the grid (or not finite), for a ``row_count`` above
        ``max_rows``, for the reductions' two bits and for the clustering's four."""
        flag = int(self.error_flag.item())
        if flag & _lib.VOXEL_ERR_RANGE:
            raise ValueError("VoxelGrid: a row has a non-finite coordinate or lies outside the grid's 2**21 cells per axis")
        if flag & _lib.VOXEL_ERR_ROWS:
            raise ValueError("VoxelGrid: a row_count is above max_rows")
        if flag & _lib.SEGMENT_ERR_NONFINITE:
            raise ValueError("VoxelGrid: a voxel's mean met a NaN or an infinity (that column of that voxel is NaN)")
        if flag & _lib.SEGMENT_ERR_RANGE:
            raise ValueError("VoxelGrid: a row names a voxel at or beyond the voxel count")
        if flag & _lib.CLUSTER_ERR_INDEX:
            raise ValueError("VoxelGrid.components: a voxel names a row outside its cloud, or a row a voxel at or beyond the voxel count")
        if flag & _lib.CLUSTER_ERR_CELL:
            raise ValueError("VoxelGrid.components: a voxel's representative row lies outside the grid (or is not finite)")
        if flag & _lib.CLUSTER_ERR_CAP:
            raise ValueError("VoxelGrid.components: a walk of the component forest hit its cap: the result is not to be used")
        if flag & _lib.CLUSTER_ERR_ROWS:
            raise ValueError("VoxelGrid.components: a voxel count or row_count is above max_rows")


def euclidean_cluster(points, labels=None, voxel_size=0.1, origin=0.0, label_reduce="mode", connectivity=26, same_label=True, member=None,
                      min_points=1, min_voxels=1, row_begin=None, row_count=None, max_rows=None):
    """Euclidean clustering in one call: ``VoxelGrid(voxel_size, origin, label_reduce=).downsample(points, labels, ...)``, then
    ``components`` with ``row_labels=labels``.  ``points``: float32 ``[M, ld]`` on the device (one cloud, or B clouds back to back with
    ``row_begin`` / ``row_count`` / ``max_rows``) or ``[B, M, ld]``; ``labels``: int32 per row or None (then every voxel takes part and
    ``member`` must be None).  Returns ``(components, down, grid)``: the ``Components``, what ``downsample`` returned and the grid (its
    ``check()`` reads the error bits back).  A row's instance id is ``components.row_component``; every call allocates its buffers --
    a loop over frames holds a ``VoxelGrid`` and its two buffer sets instead."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _lib.Pn2Error("euclidean_cluster: points must live on the GPU: this package has no CPU path")
    grid = VoxelGrid(voxel_size, origin, device=points.device, label_reduce=label_reduce)
    down = grid.downsample(points, labels, row_begin, row_count, max_rows)
    comps = grid.components(points, down, row_labels=labels, connectivity=connectivity, same_label=same_label, member=member,
                            min_points=min_points, min_voxels=min_voxels, row_begin=row_begin, row_count=row_count, max_rows=max_rows)
    return comps, down, grid


def expand(values, inverse, fill):
    """Every input row takes its representative's value: ``values[inverse]`` along dimension 0, ``fill`` where ``inverse < 0``.
    ``values``: ``[V, ...]`` per output voxel of ONE cloud (``inverse`` holds ranks inside its cloud), ``inverse``: int32 / int64
    ``[M]``.  One torch gather, nothing is read back.  Ranks at or beyond V must not occur (rows of ``values`` beyond the voxel
    count are never named by ``inverse``)."""
    inv = inverse.long()
    picked = values.index_select(0, inv.clamp(min=0))
    mask = (inv < 0).view((-1,) + (1,) * (values.dim() - 1))
    return picked.masked_fill(mask, fill)


def _segment_args(what, rows, inverse, count, row_begin, row_count, max_rows, out_begin, dev):
    """The batched conventions of the segment reductions: ``(inverse, count, row_begin, row_count, B, max_rows, out_begin)``.  ONE
    cloud without ``row_begin`` / ``row_count``: every row, outputs from row 0."""
    if not inverse.is_cuda or inverse.dtype != torch.int32 or inverse.numel() != rows or not inverse.is_contiguous():
        raise ValueError("%s: inverse must be a contiguous int32 device tensor, one entry per row" % what)
    if (row_begin is None) != (row_count is None):
        raise ValueError("%s: row_begin and row_count go together" % what)
    if not isinstance(count, torch.Tensor):
        count = torch.full((1,), int(count), device=dev, dtype=torch.int64)
    count = count.reshape(-1)
    B = int(count.numel())
    if row_begin is None:
        if B != 1:
            raise ValueError("%s: several clouds need row_begin and row_count" % what)
        row_begin = torch.zeros(1, device=dev, dtype=torch.int64)
        row_count = torch.full((1,), rows, device=dev, dtype=torch.int64)
    out_begin = row_begin if out_begin is None else out_begin
    for t in (count, row_begin, row_count, out_begin):
        if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
            raise ValueError("%s: count, row_begin, row_count and out_begin must be int64 [B] device tensors" % what)
    return inverse, count, row_begin, row_count, B, (rows if max_rows is None else int(max_rows)), out_begin


def _values_2d(what, values):
    if not isinstance(values, torch.Tensor) or not values.is_cuda:
        raise _lib.Pn2Error("%s: the values must live on the GPU: this package has no CPU path" % what)
    if values.dtype != torch.float32 or values.dim() != 2 or not 1 <= values.shape[1] <= _lib.SEGMENT_MAX_COLS or not values.is_contiguous():
        raise ValueError("%s: a contiguous float32 [rows, C] tensor, 1 <= C <= %d" % (what, _lib.SEGMENT_MAX_COLS))
    return int(values.shape[0]), int(values.shape[1])


def _workspace(workspace, B, max_rows, C, dev):
    nbytes = _lib.workspace_bytes("pn2_segment_reduce_workspace_bytes", (B, max_rows, C), _lib.Pn2Error,
                                  "segment reduction: B = %d, max_rows = %d, C = %d are not supported" % (B, max_rows, C))
    if workspace is None:
        return torch.empty(nbytes, device=dev, dtype=torch.uint8)
    if not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < nbytes:
        raise ValueError("segment reduction: the workspace must be a uint8 device tensor of at least %d bytes" % nbytes)
    return workspace


def segment_mean(values, inverse, count, n_points=None, row_begin=None, row_count=None, max_rows=None, out_begin=None, out_rows=None,
                 out=None, n_out=None, error_flag=None, workspace=None):
    """The mean of ``values``' rows per segment (``pn2_segment_mean``; the rule of include/pn2.h: a 64-bit integer sum of fixed-point
    terms, so the result does not depend on the order of the rows and is byte-identical from run to run).

    ``values``: float32 ``[rows, C]`` on the device, C <= 16; ``inverse``: int32 ``[rows]``, the segment (rank inside its cloud) of
    every row, negative = the row takes no part; ``count``: the number of segments, an int or an int64 ``[B]`` DEVICE tensor
    (``VoxelGrid.downsample``'s ``count``); ``n_points``: int32, the rows per segment (``downsample``'s) or None (counted here).
    One cloud, or B clouds with ``row_begin`` / ``row_count`` / ``max_rows`` / ``out_begin`` as ``VoxelGrid.downsample`` takes them.
    Returns float32 ``[out_rows, C]`` (default ``rows``; ``out``: a tensor to write into): segment s of cloud b is row
    ``out_begin[b] + s``; rows at or beyond the count are not written (zeros in a tensor made here).  ``n_out`` (int32): receives the
    rows per segment that were used.  ``error_flag`` (device int32, not cleared here) collects ``_lib.SEGMENT_ERR_*``.  With ``out``,
    ``workspace`` (``pn2_segment_reduce_workspace_bytes``) and device-side counts the call allocates nothing and can be captured."""
    rows, C = _values_2d("segment_mean", values)
    dev = values.device
    inverse, count, row_begin, row_count, B, max_rows, out_begin = _segment_args("segment_mean", rows, inverse, count, row_begin, row_count,
                                                                                max_rows, out_begin, dev)
    if out is None:
        out = torch.zeros(rows if out_rows is None else int(out_rows), C, device=dev, dtype=torch.float32)
    elif not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != C or not out.is_contiguous():
        raise ValueError("segment_mean: out must be a contiguous float32 [out_rows, C] device tensor")
    p = _lib.ptr
    _lib.check(_lib.load().pn2_segment_mean(p(values), C, C, p(inverse), p(row_begin), p(row_count), B, max_rows, p(out_begin), p(count),
                                            p(n_points), p(out), C, p(n_out), p(error_flag), p(_workspace(workspace, B, max_rows, C, dev)),
                                            _lib.stream()), "pn2_segment_mean")
    return out


def segment_mode(labels, inverse, count, fill=-1, return_votes=False, row_begin=None, row_count=None, max_rows=None, out_begin=None,
                 out_rows=None, out=None, votes=None, error_flag=None, workspace=None):
    """The majority label per segment (``pn2_segment_mode``): of the rows that take part and carry a label >= 0 the label with the
    most votes, the LOWEST label among equals, ``fill`` for a segment without a voter.  ``labels``: int32 ``[rows]`` on the device;
    the other arguments as ``segment_mean``'s.  Returns int32 ``[out_rows]`` (rows at or beyond the count hold ``fill`` in a tensor
    made here), with ``return_votes`` also the winners' counts (``votes / n_points`` is a cell's purity).  Integer arithmetic, no class
    limit: the result is identical from run to run."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise _lib.Pn2Error("segment_mode: the labels must live on the GPU: this package has no CPU path")
    if labels.dtype != torch.int32 or labels.dim() != 1 or not labels.is_contiguous():
        raise ValueError("segment_mode: labels must be a contiguous int32 [rows] device tensor")
    rows, dev = int(labels.numel()), labels.device
    inverse, count, row_begin, row_count, B, max_rows, out_begin = _segment_args("segment_mode", rows, inverse, count, row_begin, row_count,
                                                                                max_rows, out_begin, dev)
    n_out = rows if out_rows is None else int(out_rows)
    if out is None:
        out = torch.full((n_out,), int(fill), device=dev, dtype=torch.int32)
    if votes is None and return_votes:
        votes = torch.zeros(n_out, device=dev, dtype=torch.int32)
    p = _lib.ptr
    _lib.check(_lib.load().pn2_segment_mode(p(labels), p(inverse), p(row_begin), p(row_count), B, max_rows, p(out_begin), p(count), int(fill),
                                            p(out), p(votes), p(error_flag), p(_workspace(workspace, B, max_rows, 1, dev)), _lib.stream()),
               "pn2_segment_mode")
    return (out, votes) if return_votes else out


class _PoolMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, inverse, count, n_points, row_begin, row_count, max_rows, out_begin, out_rows, error_flag):
        rows, C = _values_2d("pool_mean", values)
        dev = values.device
        inverse, count, row_begin, row_count, B, max_rows, out_begin = _segment_args("pool_mean", rows, inverse, count, row_begin, row_count,
                                                                                    max_rows, out_begin, dev)
        out_rows = rows if out_rows is None else int(out_rows)
        n_used = torch.zeros(out_rows, device=dev, dtype=torch.int32)
        out = segment_mean(values, inverse, count, n_points, row_begin, row_count, max_rows, out_begin, out_rows, n_out=n_used,
                           error_flag=error_flag)
        ctx.save_for_backward(inverse, count, row_begin, row_count, out_begin, n_used)
        ctx.shape = (rows, C, B, max_rows)
        ctx.error_flag = error_flag
        return out

    @staticmethod
    def backward(ctx, grad_out):
        inverse, count, row_begin, row_count, out_begin, n_used = ctx.saved_tensors
        rows, C, B, max_rows = ctx.shape
        grad_out = grad_out.contiguous()
        grad_in = torch.zeros(rows, C, device=grad_out.device, dtype=torch.float32)      # (rows outside the clouds are not written)
        p = _lib.ptr
        _lib.check(_lib.load().pn2_segment_mean_bwd(p(grad_out), C, C, p(inverse), p(row_begin), p(row_count), B, max_rows, p(out_begin),
                                                    p(count), p(n_used), p(grad_in), C, p(ctx.error_flag), _lib.stream()),
                   "pn2_segment_mean_bwd")
        return (grad_in,) + (None,) * 9


def pool_mean(values, inverse, count, n_points=None, row_begin=None, row_count=None, max_rows=None, out_begin=None, out_rows=None,
              error_flag=None):
    """``segment_mean`` as a ``torch.autograd.Function`` on the two mean kernels: per-point features ``[rows, C]`` pooled to their
    voxels inside a model and trained through.  Forward ``pn2_segment_mean``, backward ``pn2_segment_mean_bwd``
    (``grad_in[row] = grad_out[segment of row] / float32(n)``, zeros for a row that takes no part).  Arguments as ``segment_mean``'s;
    features wider than 16 columns are pooled 16 columns at a time by the caller."""
    return _PoolMean.apply(values, inverse, count, n_points, row_begin, row_count, max_rows, out_begin, out_rows, error_flag)
