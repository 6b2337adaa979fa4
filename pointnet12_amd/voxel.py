"""Voxel-grid downsampling on the device (``pn2_voxel_grid``, csrc/voxel.hip): one row per occupied cell of a regular grid.

The grid subsample of every LiDAR code base: of the rows that fall into one cell the one with the lowest row number is kept, the
kept rows stay in the cloud's order (a stable compaction, ``np.sort(np.unique(key, return_index=True)[1])``), and every input
row learns which output row stands for it (``inverse``).  The kept COUNT stays in device memory, where ``pn2_prepare_clouds`` and
the device-side choice read it; nothing is read back or allocated by a call with ``out=``, so it captures into a graph, and the
result is byte-identical from run to run.  The rule is stated in include/pn2.h (and, in numpy, in tests/voxel_ref.py).

Out of scope: the MEAN of a voxel's rows (a run-to-run identical mean needs a fixed-order segmented sum; ``inverse`` and
``n_points`` are what it would be built from) and grids over more than three key columns.
"""
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
    ``labels`` / ``index`` / ``inverse`` / ``n_points`` int32 ``[rows]``, ``count`` int64 ``[B]`` and the kernel's ``workspace``."""

    def __init__(self, rows, B, max_rows, ld, device):
        nbytes = _lib.load().pn2_voxel_grid_workspace_bytes(int(B), int(max_rows))
        if nbytes < 0:
            raise _lib.Pn2Error("VoxelBuffers: B = %d, max_rows = %d are not supported" % (B, max_rows))
        self.rows, self.B, self.max_rows, self.ld = int(rows), int(B), int(max_rows), int(ld)
        i32 = lambda: torch.empty(self.rows, device=device, dtype=torch.int32)
        self.points = torch.empty(self.rows, self.ld, device=device, dtype=torch.float32)
        self.labels, self.index, self.inverse, self.n_points = i32(), i32(), i32(), i32()
        self.count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)


class VoxelGrid:
    """A regular grid of cells ``voxel_size`` wide (a scalar or one size per axis) whose cell 0 starts at ``origin`` (likewise):
    a point p lies in cell ``floor((float64(p) - origin) / voxel_size)`` per axis, and cells from -2**20 to 2**20 - 1 exist.

    ``error_flag`` (device int32, cleared at the start of every ``downsample``) collects ``_lib.VOXEL_ERR_RANGE`` (a row with a
    non-finite coordinate or outside the grid: it is dropped and its ``inverse`` is -1) and ``_lib.VOXEL_ERR_ROWS`` (a
    ``row_count`` above ``max_rows``: the rows beyond are ignored); ``check()`` reads it back and raises ``ValueError``."""

    def __init__(self, voxel_size, origin=0.0, device="cuda"):
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
        return VoxelBuffers(rows, B, rows if max_rows is None else max_rows, ld, self.device)

    def downsample(self, points, labels=None, row_begin=None, row_count=None, max_rows=None, out=None, out_begin=None):
        """``(points, labels, index, count, inverse, n_points)`` as device tensors.  ``points``: float32 on the device, ``[M, ld]``
        (one cloud, or B clouds back to back with ``row_begin`` / ``row_count``: int64 ``[B]`` DEVICE tensors as
        ``pn2_prepare_clouds`` reads them) or ``[B, M, ld]`` contiguous (``row_begin`` = b * M and ``row_count`` = M unless
        given), 3 <= ld <= 16, columns 0..2 = x, y, z.  ``labels``: int32 ``[rows]`` or None (``labels`` of the result is then None).
        ``max_rows``: a host bound of every count (None: M).

        Cloud b's voxels are rows ``out_begin[b] : out_begin[b] + count[b]`` of the outputs (``out_begin``: int64 ``[B]`` on the
        device, None: ``row_begin``), in the order of their representatives -- each voxel's lowest row: ``points`` (that row, all
        ``ld`` floats bit for bit), ``labels`` (its label), ``index`` int32 (its row inside the cloud, strictly increasing) and
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
            held = getattr(self, "_regular", None)                   # (kept: a second call of the same shape allocates nothing)
            if held is None or held[0] != (points.dim(), int(points.shape[0]), M):
                nb = 1 if points.dim() == 2 else int(points.shape[0])
                held = self._regular = ((points.dim(), int(points.shape[0]), M),
                                        torch.arange(nb, device=self.device, dtype=torch.int64) * M,
                                        torch.full((nb,), M, device=self.device, dtype=torch.int64))
            row_begin, row_count = held[1], held[2]
        B = int(row_begin.numel())
        for t in (row_begin, row_count) + (() if out_begin is None else (out_begin,)):
            if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
                raise ValueError("VoxelGrid.downsample: row_begin, row_count and out_begin must be int64 [B] device tensors")
        max_rows = M if max_rows is None else int(max_rows)
        if out is None:
            out = VoxelBuffers(rows, B, max_rows, ld, self.device)
        elif out.B != B or out.max_rows < max_rows or out.ld != ld or out.rows < rows:
            raise ValueError("VoxelGrid.downsample: out was made for B = %d, max_rows = %d, ld = %d, %d rows"
                             % (out.B, out.max_rows, out.ld, out.rows))
        p = _lib.ptr
        dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self.error_flag.zero_()                                      # an async fill, nothing is read back
        # (max_rows as the buffers were made for: the workspace layout follows it)
        _lib.check(_lib.load().pn2_voxel_grid(p(points), ld, p(labels), p(row_begin), p(row_count), B, out.max_rows, dp(self.origin),
                                              dp(self.voxel_size), p(row_begin if out_begin is None else out_begin), p(out.points),
                                              p(out.labels) if labels is not None else None, p(out.index), p(out.count),
                                              p(out.inverse), p(out.n_points), p(self.error_flag), p(out.workspace), _lib.stream()),
                   "pn2_voxel_grid")
        return out.points, (out.labels if labels is not None else None), out.index, out.count, out.inverse, out.n_points

    def check(self):
        """Reads ``error_flag`` back: ``ValueError`` for a row outside the grid (or not finite) and for a ``row_count`` above
        ``max_rows``."""
        flag = int(self.error_flag.item())
        if flag & _lib.VOXEL_ERR_RANGE:
            raise ValueError("VoxelGrid: a row has a non-finite coordinate or lies outside the grid's 2**21 cells per axis")
        if flag & _lib.VOXEL_ERR_ROWS:
            raise ValueError("VoxelGrid: a row_count is above max_rows")


def expand(values, inverse, fill):
    """Every input row takes its representative's value: ``values[inverse]`` along dimension 0, ``fill`` where ``inverse < 0``.
    ``values``: ``[V, ...]`` per output voxel of ONE cloud (``inverse`` holds ranks inside its cloud), ``inverse``: int32 / int64
    ``[M]``.  One torch gather, nothing is read back.  Ranks at or beyond V must not occur (rows of ``values`` beyond the voxel
    count are never named by ``inverse``)."""
    inv = inverse.long()
    picked = values.index_select(0, inv.clamp(min=0))
    mask = (inv < 0).view((-1,) + (1,) * (values.dim() - 1))
    return picked.masked_fill(mask, fill)
