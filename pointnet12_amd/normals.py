"""Surface normals and local PCA over neighbour lists: ``pn2_local_pca`` (csrc/normals.hip; the rule is stated in include/pn2.h
under "local PCA" and in numpy in tests/normals_ref.py).

The reference repository has no such function: like kNN, the voxel grid, clustering and Lovasz this is an extension.  For every
point, the covariance of its neighbourhood (fp64, one pass), its three eigenvalues ``l0 <= l1 <= l2`` and the unit eigenvector
of ``l0`` -- which way the surface faces, and how flat it is.  OUT OF SCOPE: a gradient through the normals; a consistent
orientation by propagation along a spanning tree (the sign is per point: towards a viewpoint, or +z, +y, +x); weighted
neighbourhoods.  (``estimate_normals`` searches with ``pn2_knn``'s brute force by default; ``search="grid"`` takes the uniform grid of
``neighbors.GridIndex`` instead, which is what a whole scan needs.)
"""
import numpy as np
import torch

from . import _lib, neighbors

_p = _lib.ptr


def _points(t, name):
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


class NormalBuffers:
    """Everything ``estimate_normals`` / ``local_pca`` write, allocated once (``buffers``).  ``normal`` float32 [B,N,3], ``eig``
    float32 [B,N,3], ``cov`` float64 [B,N,6] (xx, xy, xz, yy, yz, zz), ``count`` int32 [B,N]; ``xyz`` / ``idx`` / ``dist``: the
    packed copy and the neighbour lists of ``estimate_normals``; ``origin``: a zero viewpoint.  ``grid`` (``search="grid"``): the
    ``neighbors.GridBuffers`` of the grid search, whose ``idx`` / ``dist`` these then are.  ``error_flag`` (device int32,
    cleared at the start of every call that is given these buffers) collects ``_lib.PCA_ERR_FEW`` (a row with fewer than three
    valid neighbours: its normal is zero) and ``_lib.PCA_ERR_NONFINITE`` (a NaN / inf point: the row holds NaN)."""

    def __init__(self, N, B, k, device, cov=True, search="brute"):
        self.B, self.N, self.k = int(B), int(N), int(k)
        self.xyz = torch.zeros(B, N, 3, device=device, dtype=torch.float32)
        self.device = self.xyz.device                                # ("cuda" resolved to the current device's index)
        self.grid = None
        if search == "grid":
            self.grid = neighbors.GridBuffers(N, B, N, k, self.device)
            self.idx, self.dist = self.grid.idx, self.grid.dist
        elif search == "brute":
            self.idx = torch.zeros(B, N, k, device=device, dtype=torch.int64)
            self.dist = torch.zeros(B, N, k, device=device, dtype=torch.float32)
        else:
            raise ValueError("normals.buffers: search must be \"brute\" or \"grid\"")
        self.normal = torch.zeros(B, N, 3, device=device, dtype=torch.float32)
        self.eig = torch.zeros(B, N, 3, device=device, dtype=torch.float32)
        self.cov = torch.zeros(B, N, 6, device=device, dtype=torch.float64) if cov else None
        self.count = torch.zeros(B, N, device=device, dtype=torch.int32)
        self.origin = torch.zeros(B, 3, device=device, dtype=torch.float32)
        self.error_flag = torch.zeros(1, device=device, dtype=torch.int32)

    def check(self, few_ok=True):
        """Reads ``error_flag`` back: ``ValueError`` for a point that is not finite, and, unless ``few_ok`` (an isolated point
        under a radius is ordinary in a scan), for a row with fewer than three valid neighbours."""
        flag = int(self.error_flag.item())
        if flag & _lib.PCA_ERR_NONFINITE:
            raise ValueError("local_pca: a neighbour (or, with a viewpoint, a query point) is not finite; those rows hold NaN")
        if flag & _lib.PCA_ERR_FEW and not few_ok:
            raise ValueError("local_pca: a row has fewer than three valid neighbours; its normal is zero")


def buffers(N, B=1, k=16, device="cuda", cov=True, search="brute"):
    """Preallocates for ``N`` rows per cloud, ``B`` clouds and ``k`` neighbours.  With ``buffers=`` a call allocates nothing, reads
    nothing back and captures into a graph that stays valid when the device-side counts (``n_points`` / ``n_query``) change.
    (A ``viewpoint`` must then be a device tensor or ``"origin"``: a host triple would be copied in.)  ``search="grid"`` adds the grid
    search's workspace (``estimate_normals(search="grid")`` needs it; the brute-force search runs on such buffers too)."""
    return NormalBuffers(N, B, k, device, cov, search)


def _viewpoint(v, B, dev, buf, what):
    if v is None:
        return None
    if isinstance(v, str):
        if v != "origin":
            raise ValueError("%s: viewpoint must be a triple, a [B, 3] tensor or \"origin\"" % what)
        return buf.origin if buf is not None else torch.zeros(B, 3, device=dev, dtype=torch.float32)
    if isinstance(v, torch.Tensor):
        if not v.is_cuda or v.dtype != torch.float32 or v.numel() != 3 * B:
            raise ValueError("%s: a viewpoint tensor must be float32 [B, 3] on the GPU" % what)
        return v.reshape(B, 3).contiguous()
    t = torch.as_tensor(np.asarray(v, np.float32).reshape(-1), dtype=torch.float32)
    if t.numel() != 3:
        raise ValueError("%s: a viewpoint triple has three entries" % what)
    return t.to(dev).reshape(1, 3).repeat(B, 1).contiguous()


def local_pca(points, idx, dist=None, query=None, max_dist=None, viewpoint=None, n_query=None, out=None, out_col=0, return_eig=False,
              return_cov=False, return_count=False, err=None, buffers=None):
    """Normals (and on request eigenvalues, covariance and neighbour count) of the neighbourhoods ``idx`` lists.

    ``points`` [B,M,ld] (or [M,ld]) float32, 3 <= ld <= 16, columns 0..2 = x, y, z, read where they lie; ``idx`` int64 [B,N,K] as
    ``knn_point`` or ``query_ball_point`` return it; ``dist`` float32 [B,N,K] squared distances or None.  A slot counts iff
    ``0 <= idx < M`` and not ``dist > float32(max_dist ** 2)`` (``max_dist`` in the units of the points; None: no cut-off); a
    candidate listed several times counts once per appearance.  Covariance with divisor n; ``l0 <= l1 <= l2`` its eigenvalues;
    the normal is the unit eigenvector of ``l0``, turned towards ``viewpoint`` (a triple, a float32 [B,3] device tensor, or
    ``"origin"``) as seen from the row's ``query`` point ([B,N,ld]; default: ``points``, which then needs N == M), or, without
    one, to +z (then +y, then +x).  Fewer than three valid slots: a zero normal and ``PCA_ERR_FEW`` in ``err``; a point that is
    not finite: NaN and ``PCA_ERR_NONFINITE``.  ``n_query``: device int64 [B] (or host integers), rows at and beyond it keep
    what the outputs held (zeros when they are allocated here).

    ``out`` (float32 [B,N,C] or [N,C], contiguous) with ``out_col``: the normals go to columns ``out_col .. out_col + 2`` of an
    existing row buffer, nothing else in it is touched.  Returns the normals ([B,N,3] or [N,3]; ``out`` when given), followed
    by ``eig`` float32 [.,3], ``cov`` float64 [.,6] (xx, xy, xz, yy, yz, zz), ``count`` int32 [.] as asked for.  ``err``: a zeroed
    device int32 tensor, nothing is read back here.  ``buffers``: a ``NormalBuffers``; the outputs then live there."""
    flat = isinstance(points, torch.Tensor) and points.dim() == 2
    points = _points(points, "points")
    B, M, ldc = points.shape
    dev = points.device
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype != torch.int64 or idx.dim() != (2 if flat else 3):
        raise ValueError("local_pca: idx must be an int64 [B, N, K] tensor on the GPU ([N, K] for [M, ld] points)")
    idx = idx.contiguous()
    idx = idx[None] if flat else idx
    if idx.shape[0] != B:
        raise ValueError("local_pca: idx and points disagree on B")
    _, N, K = idx.shape
    if dist is not None:
        if not dist.is_cuda or dist.dtype != torch.float32 or dist.numel() != idx.numel():
            raise ValueError("local_pca: dist must be float32 of idx's shape on the GPU")
        dist = dist.contiguous()
    buf = buffers
    if buf is not None and (buf.B != B or buf.N != N or buf.device != dev):
        raise ValueError("local_pca: the buffers were made for B = %d, N = %d on %s" % (buf.B, buf.N, buf.device))
    if query is not None:
        query = _points(query, "query")
        if query.shape[0] != B or query.shape[1] != N:
            raise ValueError("local_pca: query must be [B, N, ld]")
    elif viewpoint is not None:
        if N != M:
            raise ValueError("local_pca: a viewpoint needs the query points (query=) unless idx has a row per point")
        query = points
    vp = _viewpoint(viewpoint, B, dev, buf, "local_pca")
    n_query = _counts(n_query, B, dev, "local_pca: n_query")
    if err is None and buf is not None:
        err = buf.error_flag
        err.zero_()                                              # an async fill, nothing is read back
    if err is not None and (not err.is_cuda or err.dtype != torch.int32 or err.numel() < 1):
        raise ValueError("local_pca: err must be a device int32 tensor")

    def alloc(name, cols, dtype, want):
        if not want:
            return None
        if buf is not None:
            if getattr(buf, name) is None:
                raise ValueError("local_pca: the buffers hold no %s" % name)
            return getattr(buf, name)
        make = torch.zeros if n_query is not None else torch.empty
        return make((B, N, cols) if cols else (B, N), device=dev, dtype=dtype)

    if out is not None:
        if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != (2 if flat else 3) or \
                out.numel() % (B * N) != 0 or out.shape[-2] != N:
            raise ValueError("local_pca: out must be a contiguous float32 [B, N, C] tensor on the GPU")
        ldn = out.shape[-1]
        out_col = int(out_col)
        if out_col < 0 or out_col + 3 > ldn:
            raise ValueError("local_pca: columns %d .. %d do not fit a row of %d" % (out_col, out_col + 2, ldn))
        normal_ptr = out.data_ptr() + 4 * out_col
        normal = out
    else:
        normal = alloc("normal", 3, torch.float32, True)
        ldn, normal_ptr = 3, normal.data_ptr()
    eig = alloc("eig", 3, torch.float32, return_eig)
    cov = alloc("cov", 6, torch.float64, return_cov)
    count = alloc("count", 0, torch.int32, return_count)
    max_d2 = float("inf") if max_dist is None else float(np.float32(float(max_dist) ** 2))
    _lib.check(_lib.load().pn2_local_pca(_p(query), 0 if query is None else query.shape[2], _p(points), ldc, _p(idx), _p(dist), B, N, M, K,
                                         max_d2, _p(n_query), _p(vp), normal_ptr, ldn, _p(eig), _p(cov), _p(count), _p(err),
                                         _lib.stream()), "pn2_local_pca")
    res = [normal if out is not None else (normal[0] if flat else normal)]
    for t, want in ((eig, return_eig), (cov, return_cov)):
        if want:
            res.append(t[0] if flat else t)
    if return_count:
        res.append(count[0] if flat else count)
    return res[0] if len(res) == 1 else tuple(res)


def estimate_normals(points, k=16, radius=None, viewpoint=None, n_points=None, out=None, out_col=0, return_eig=False, return_cov=False,
                     return_count=False, err=None, buffers=None, search="brute"):
    """Normals of a cloud from its own points: a self-search for the ``min(k, M)`` nearest neighbours (``pn2_knn``; the point itself
    is one of them), of which those within ``radius`` count -- the "k nearest within r" search normal estimation conventionally
    uses -- then ``local_pca``.  ``points`` [M,ld] or [B,M,ld] float32 (a [., 4] scan as it lies; one packed xyz copy is made
    for the search).  ``viewpoint``: a triple, a float32 [B,3] device tensor, or ``"origin"`` (the scanner of a KITTI scan).
    ``n_points``: device int64 [B] (or host integers), only that many leading rows of each cloud are searched and written.
    The other arguments and the return value are ``local_pca``'s.

    BY DEFAULT THE SEARCH IS BRUTE FORCE (M x M pairs: a 120 000-row scan against itself is 1.4e10).  ``search="grid"`` bins the
    cloud on a uniform grid of cells one ``radius`` wide first (``neighbors.GridIndex``; it needs a ``radius``, else
    ``ValueError``) and looks at 27 cells per row: the [., ld] rows are read where they lie, no packed copy is made, and the
    neighbour lists go to ``local_pca`` with the same cut-off.  Its distances are in difference form, ``pn2_knn``'s in expanded
    form: off a lattice the two may order near-ties differently, and a row that is not finite finds no neighbours
    (``PCA_ERR_FEW``) instead of poisoning its own (``PCA_ERR_NONFINITE``).  ``k`` above ``_lib.KNN_MAX_K`` raises."""
    if search not in ("brute", "grid"):
        raise ValueError("estimate_normals: search must be \"brute\" or \"grid\"")
    if search == "grid" and radius is None:
        raise ValueError("estimate_normals: search=\"grid\" needs a radius (the grid's cell)")
    flat = isinstance(points, torch.Tensor) and points.dim() == 2
    pts = _points(points, "points")
    B, M, _ = pts.shape
    dev = pts.device
    k = min(int(k), M)
    if k < 1:
        raise RuntimeError("estimate_normals: k must be at least 1")
    if k > _lib.KNN_MAX_K:
        raise RuntimeError("estimate_normals: k (%d) > %d is not supported (there is no fallback path)" % (k, _lib.KNN_MAX_K))
    buf = buffers
    if buf is not None and (buf.B != B or buf.N != M or buf.k < k or buf.device != dev):
        raise ValueError("estimate_normals: the buffers were made for B = %d, N = %d, k >= %d on %s" % (buf.B, buf.N, buf.k, buf.device))
    n_points = _counts(n_points, B, dev, "estimate_normals: n_points")
    if search == "grid":
        if buf is not None and buf.grid is None:
            raise ValueError("estimate_normals: these buffers hold no grid workspace (normals.buffers(..., search=\"grid\"))")
        index = neighbors.GridIndex(radius=radius).build(pts, n_cand=n_points, buffers=None if buf is None else buf.grid)
        idx, dist = index.query_self(k, return_dist=True, buffers=None if buf is None else buf.grid)
        xyz = pts
    elif buf is not None:
        xyz = buf.xyz
        xyz.copy_(pts[:, :, :3])
        idx = buf.idx.reshape(-1)[:B * M * k].reshape(B, M, k)
        dist = buf.dist.reshape(-1)[:B * M * k].reshape(B, M, k)
    else:
        xyz = pts[:, :, :3].contiguous()
        idx = torch.empty(B, M, k, device=dev, dtype=torch.int64)
        dist = torch.empty(B, M, k, device=dev, dtype=torch.float32)
    if search == "brute":
        _lib.check(_lib.load().pn2_knn(_p(xyz), _p(xyz), B, M, M, k, _p(n_points), _p(n_points), _p(idx), _p(dist), _lib.stream()),
                   "pn2_knn")
    res = local_pca(xyz, idx, dist, query=xyz, max_dist=radius, viewpoint=viewpoint, n_query=n_points,
                    out=out if (out is None or not flat) else out[None], out_col=out_col, return_eig=return_eig, return_cov=return_cov,
                    return_count=return_count, err=err, buffers=buf)
    if not flat:
        return res
    if isinstance(res, tuple):
        return tuple(out if (i == 0 and out is not None) else r[0] for i, r in enumerate(res))
    return out if out is not None else res[0]


def surface_variation(eig):
    """``l0 / ((l0 + l1) + l2)`` of ``eig`` [..., 3] (ascending eigenvalues), and 0 where the sum is 0: 0 on a plane, 1/3 where the
    neighbourhood is isotropic (Pauly et al.'s surface variation).  Plain torch on the float32 eigenvalues."""
    s = (eig[..., 0] + eig[..., 1]) + eig[..., 2]
    return torch.where(s > 0, eig[..., 0] / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))


def eigen_features(eig):
    """``(linearity, planarity, sphericity) = ((l2 - l1) / l2, (l1 - l0) / l2, l0 / l2)`` of ``eig`` [..., 3] (ascending
    eigenvalues; they add up to 1), each 0 where ``l2`` is 0.  Plain torch on the float32 eigenvalues."""
    l0, l1, l2 = eig[..., 0], eig[..., 1], eig[..., 2]
    pos = l2 > 0
    d = torch.where(pos, l2, torch.ones_like(l2))
    z = torch.zeros_like(l2)
    return torch.where(pos, (l2 - l1) / d, z), torch.where(pos, (l1 - l0) / d, z), torch.where(pos, l0 / d, z)
