"""Grid-accelerated "k nearest within r": ``pn2_grid_build`` / ``pn2_grid_knn`` (csrc/grid_knn.hip; the rule is stated in
include/pn2.h under "grid kNN" and in numpy in tests/grid_knn_ref.py).

The reference repository has no such function: like kNN, the voxel grid, clustering and normals this is an extension.  The
candidates are binned by cell once (``GridIndex.build``); every query then looks at the 27 cells around its own.  With the default
cell -- ``sqrt(float64(max_d2)) * (1 + 2**-20)``, a hair above the radius -- the result EQUALS the brute-force "k nearest with
``d2 <= max_d2``" in the same float32 difference-form arithmetic ("Grid kNN"); a smaller cell is refused.  ``idx`` /
``dist`` have ``knn_point``'s layout and padding (``idx = M``, ``dist = +inf``) and feed ``pn2_knn_vote`` and ``local_pca``
unchanged.  OUT OF SCOPE: a reach beyond 27 cells, a grid ball query, kNN without a radius, a gradient.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_p = _lib.ptr

# Which way a self-search visits its rows unless told otherwise: lane i serves the i-th RECORD of the cell-sorted copy
# (PN2_GRID_VISIT_SORTED), not row i.  Same bytes either way; tools/bench_neighbors.py times both (README.md, grid kNN bullet).
SELF_VISIT_SORTED = True


def _cloud(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.Pn2Error("%s must live on the GPU: this package has no CPU path" % name)
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be float32 (got %s)" % (name, t.dtype))
    if t.dim() not in (2, 3) or not 3 <= t.shape[-1] <= 16:
        raise RuntimeError("%s must be [M, ld] or [B, M, ld] with 3 <= ld <= 16 (columns 0..2 = x, y, z)" % name)
    t = t.contiguous()
    return t if t.dim() == 3 else t[None]


def _counts(n, B, device, what):
    if n is None:
        return None
    if not isinstance(n, torch.Tensor):
        n = torch.as_tensor(n, dtype=torch.int64).reshape(-1).to(device)
    if not n.is_cuda or n.dtype != torch.int64 or n.numel() != B:
        raise ValueError("%s must hold B = %d int64 counts on the GPU" % (what, B))
    return n.reshape(-1).contiguous()


def _triple(v, what):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3 or not np.isfinite(a).all():
        raise ValueError("GridIndex: %s must be a finite number or triple" % what)
    return a


def workspace_bytes(M, B=1):
    """Bytes of the workspace ``pn2_grid_build`` fills for ``B`` clouds of up to ``M`` candidates (host-only call)."""
    return _lib.workspace_bytes("pn2_grid_workspace_bytes", (int(B), int(M)), ValueError,
                                "GridIndex: B = %d clouds of M = %d rows are not supported" % (B, M))


class GridBuffers:
    """Everything ``GridIndex.build`` / ``query`` / ``query_self`` write, allocated once (``GridIndex.buffers``): the persistent
    ``workspace`` (uint8), ``idx`` int64 [B,N,k], ``dist`` float32 [B,N,k], ``count`` int32 [B,N].  ``error_flag`` (device int32,
    cleared at the start of every ``build`` that is given these buffers; the searches OR into it) collects ``_lib.GRID_ERR_CAND``
    (a candidate that is not finite or lies outside the grid: never returned) and ``_lib.GRID_ERR_QUERY`` (such a query: its
    row is empty)."""

    def __init__(self, M, B, N, k, device):
        self.B, self.M, self.N, self.k = int(B), int(M), int(M if N is None else N), int(k)
        self.workspace = torch.empty(workspace_bytes(self.M, self.B), device=device, dtype=torch.uint8)
        self.device = self.workspace.device
        self.idx = torch.full((self.B, self.N, self.k), self.M, device=device, dtype=torch.int64)
        self.dist = torch.full((self.B, self.N, self.k), float("inf"), device=device, dtype=torch.float32)
        self.count = torch.zeros(self.B, self.N, device=device, dtype=torch.int32)
        self.error_flag = torch.zeros(1, device=device, dtype=torch.int32)

    def check(self):
        """Reads ``error_flag`` back: ``ValueError`` for a candidate or a query that is not finite or lies outside the grid."""
        flag = int(self.error_flag.item())
        if flag & _lib.GRID_ERR_CAND:
            raise ValueError("GridIndex: a candidate is not finite or lies outside the grid's 2^21 cells per axis; it was not indexed")
        if flag & _lib.GRID_ERR_QUERY:
            raise ValueError("GridIndex: a query is not finite or lies outside the grid's 2^21 cells per axis; its row is empty")


class GridIndex:
    """A uniform grid over candidate clouds for "k nearest within ``radius``".

    ``max_d2 = float32(radius ** 2)`` (``propagate_labels``' cut-off rule; or pass ``max_d2`` itself).  ``cell``: the cell edge, a
    number or a triple, by default ``sqrt(float64(max_d2)) * (1 + 2**-20)`` on every axis; a smaller one raises ``ValueError``
    (the search would miss in-radius candidates); ``max_d2 = inf`` ("the k nearest of the 27 cells") needs an explicit ``cell``.
    ``origin``: a corner of cell 0, a number or a triple.  The grid has 2^21 cells per axis around it.

    ``build(cand)`` once, then any number of ``query`` / ``query_self``.  With ``buffers=`` nothing is allocated and nothing is
    read back: build plus query capture into a graph that stays valid when the device-side counts and the points change."""

    def __init__(self, radius=None, max_d2=None, cell=None, origin=0.0, device="cuda"):
        if (radius is None) == (max_d2 is None):
            raise ValueError("GridIndex: give either radius or max_d2")
        m = np.float32(float(radius) ** 2) if max_d2 is None else np.float32(max_d2)
        if not m >= 0:
            raise ValueError("GridIndex: the cut-off must not be negative or NaN")
        self.max_d2 = float(m)
        if np.isinf(m):
            if cell is None:
                raise ValueError("GridIndex: max_d2 = inf needs an explicit cell")
            c = _triple(cell, "cell")
        else:
            least = float(np.sqrt(np.float64(m)) * (1.0 + 2.0 ** -20))
            c = _triple(least if cell is None else cell, "cell")
            if (c < least).any():
                raise ValueError("GridIndex: a cell edge below sqrt(max_d2) * (1 + 2**-20) = %r would miss in-radius candidates" % least)
        if not (c > 0).all():
            raise ValueError("GridIndex: cell edges must be positive")
        self.cell, self.origin = c, _triple(origin, "origin")
        self._keep = ((ctypes.c_double * 3)(*c), (ctypes.c_double * 3)(*self.origin))           # host double[3] each, alive with the index
        self._c_cell, self._c_origin = ctypes.addressof(self._keep[0]), ctypes.addressof(self._keep[1])
        self.device = device
        self.error_flag = None
        self._work = None

    def buffers(self, M, B=1, N=None, k=16):
        """Preallocates for ``B`` clouds of ``M`` candidates, ``N`` queries (default ``M``) and up to ``k`` neighbours."""
        return GridBuffers(M, B, N, k, self.device)

    def build(self, cand, n_cand=None, buffers=None):
        """Bins ``cand`` [M,ld] or [B,M,ld] float32 (3 <= ld <= 16, read where it lies).  ``n_cand``: device int64 [B] (or host
        integers), only that many leading rows of each cloud are indexed.  Returns ``self``."""
        flat = isinstance(cand, torch.Tensor) and cand.dim() == 2
        cand = _cloud(cand, "cand")
        B, M, ld = cand.shape
        dev = cand.device
        buf = buffers
        if buf is not None:
            if buf.B != B or buf.M != M or buf.device != dev:
                raise ValueError("GridIndex.build: the buffers were made for B = %d, M = %d on %s" % (buf.B, buf.M, buf.device))
            work, err = buf.workspace, buf.error_flag
            err.zero_()                                              # an async fill, nothing is read back
        else:
            work = torch.empty(workspace_bytes(M, B), device=dev, dtype=torch.uint8)
            err = torch.zeros(1, device=dev, dtype=torch.int32)
        n_cand = _counts(n_cand, B, dev, "GridIndex.build: n_cand")
        _lib.check(_lib.load().pn2_grid_build(_p(cand), ld, B, M, _p(n_cand), self._c_origin, self._c_cell, _p(err), _p(work),
                                              _lib.stream()), "pn2_grid_build")
        self._work, self.error_flag = work, err
        self._B, self._M, self._flat, self._partial, self._dev = B, M, flat, n_cand is not None, dev
        return self

    def check(self):
        """Reads the error flag of the last ``build`` (and the searches since) back; see ``GridBuffers.check``."""
        GridBuffers.check(self)

    def _search(self, query, N, ldq, k, n_query, partial, flags, return_dist, return_count, buf, flat, what):
        if self._work is None:
            raise RuntimeError("%s: build() first" % what)
        B, M, dev = self._B, self._M, self._dev
        k = int(k)
        if k < 1:
            raise RuntimeError("%s: k must be at least 1" % what)
        if k > _lib.KNN_MAX_K:
            raise RuntimeError("%s: k (%d) > %d is not supported (there is no fallback path)" % (what, k, _lib.KNN_MAX_K))
        if buf is not None:
            if buf.B != B or buf.M != M or buf.N != N or buf.k < k or buf.device != dev:
                raise ValueError("%s: the buffers were made for B = %d, M = %d, N = %d, k >= %d on %s" %
                                 (what, buf.B, buf.M, buf.N, buf.k, buf.device))
            if buf.workspace.data_ptr() != self._work.data_ptr():
                raise ValueError("%s: the index was not built into these buffers" % what)
            idx = buf.idx.reshape(-1)[:B * N * k].reshape(B, N, k)
            dist = buf.dist.reshape(-1)[:B * N * k].reshape(B, N, k) if return_dist else None
            count = buf.count if return_count else None
        else:
            # (rows at and beyond a device-side count are left untouched: they read as empty)
            idx = torch.full((B, N, k), M, device=dev, dtype=torch.int64) if partial else torch.empty(B, N, k, device=dev, dtype=torch.int64)
            dist = count = None
            if return_dist:
                dist = torch.full((B, N, k), float("inf"), device=dev) if partial else torch.empty(B, N, k, device=dev, dtype=torch.float32)
            if return_count:
                count = torch.zeros(B, N, device=dev, dtype=torch.int32) if partial else torch.empty(B, N, device=dev, dtype=torch.int32)
        _lib.check(_lib.load().pn2_grid_knn(_p(query), ldq, B, N, M, k, self.max_d2, _p(n_query), self._c_origin, self._c_cell,
                                            _p(self._work), flags, _p(idx), _p(dist), _p(count), _p(self.error_flag), _lib.stream()),
                   "pn2_grid_knn")
        res = [t[0] if flat else t for t in (idx, dist, count) if t is not None]
        return res[0] if len(res) == 1 else tuple(res)

    def query(self, query, k, n_query=None, return_dist=False, return_count=False, buffers=None):
        """The ``k`` nearest indexed candidates within the radius of every row of ``query`` [N,ld] or [B,N,ld] -> int64 [B,N,k]
        (ascending ``(d2, index)``; unfilled slots hold ``M``), followed on request by ``dist`` float32 [B,N,k] (squared, ``+inf``
        in unfilled slots) and ``count`` int32 [B,N] (candidates within the radius, not capped by ``k``).  ``n_query``: device
        int64 [B] (or host integers); the rows at and beyond it are left untouched (empty when allocated here)."""
        flat = isinstance(query, torch.Tensor) and query.dim() == 2
        query = _cloud(query, "query")
        if self._work is not None and (query.shape[0] != self._B or query.device != self._dev or flat != self._flat):
            raise ValueError("GridIndex.query: query and the indexed clouds disagree on B, the device or the number of dimensions")
        B, N, ldq = query.shape
        n_query = _counts(n_query, B, query.device, "GridIndex.query: n_query")
        return self._search(query, N, ldq, k, n_query, n_query is not None, 0, return_dist, return_count, buffers, flat, "GridIndex.query")

    def query_self(self, k, return_dist=False, return_count=False, visit_sorted=None, buffers=None):
        """``query`` with the indexed candidates as the queries (the coordinates ``build`` copied; every row finds itself at
        distance 0).  Every row below the count ``build`` read is written.  ``visit_sorted``: serve the rows in cell order
        (``PN2_GRID_VISIT_SORTED``; same bytes either way; default ``SELF_VISIT_SORTED``)."""
        if self._work is None:
            raise RuntimeError("GridIndex.query_self: build() first")
        flags = _lib.GRID_VISIT_SORTED if (SELF_VISIT_SORTED if visit_sorted is None else visit_sorted) else 0
        return self._search(None, self._M, 0, k, None, self._partial, flags, return_dist, return_count, buffers, self._flat,
                            "GridIndex.query_self")


def radius_knn(query, cand, k, radius, n_query=None, n_cand=None, return_dist=False, return_count=False, cell=None, origin=0.0):
    """Build and query in one call: the ``k`` nearest rows of ``cand`` within ``radius`` of every row of ``query`` (None: of every
    candidate itself).  See ``GridIndex.query`` for the result."""
    index = GridIndex(radius=radius, cell=cell, origin=origin).build(cand, n_cand=n_cand)
    if query is None:
        return index.query_self(k, return_dist=return_dist, return_count=return_count)
    return index.query(query, k, n_query=n_query, return_dist=return_dist, return_count=return_count)
