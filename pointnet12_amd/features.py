"""FPFH point descriptors (Fast Point Feature Histograms; Rusu, Blodow, Beetz, ICRA 2009): ``pn2_spfh`` / ``pn2_fpfh``
(csrc/fpfh.hip; the rule is stated in include/pn2.h under "FPFH" and in numpy in tests/fpfh_ref.py).

The reference repository has no such function: like kNN, the voxel grid, clustering, normals, ICP and plane fitting this is an
extension.  33 numbers per point, invariant to rigid motion, from what the package already produces: points, unit normals
(``normals.estimate_normals``) and "k nearest within r" lists (``neighbors.GridIndex.query_self`` or ``knn_point``).  The first
kernel counts three angle bins per neighbour pair into an integer row (``spfh``, a public intermediate); the second adds to every
row's own histogram the 1 / d^2 weighted mean of its neighbours' histograms.  The rule was written from the paper: it is
UNVERIFIED AGAINST OPEN3D / PCL, whose binning differs in details (include/pn2.h names the one at ties).  OUT OF SCOPE: K above 32,
PFH and SHOT, a gradient, query points other than the cloud's own.

The descriptor's consumer is here too: ``match_features`` (``pn2_feature_nn2`` / ``pn2_match_pairs``, csrc/feature_match.hip; the
rule is stated in include/pn2.h under "feature matching" and in numpy in tests/match_ref.py) gives every source row its two nearest
target rows in feature space by an exact all-pairs search, and keeps the rows that pass a mutual and a ratio test as a compacted
pair list -- what ``registration.ransac_correspondences`` and ``registration.register_global`` take.  OUT OF SCOPE there: features
wider than 64 columns, approximate or tree search in feature space, a gradient.
"""
import collections

import numpy as np
import torch

from . import _lib, neighbors
from . import normals as _normals

_p = _lib.ptr
_points = _normals._points
_counts = _normals._counts


class FpfhBuffers:
    """Everything ``spfh`` / ``fpfh`` / ``compute_fpfh`` write, allocated once (``buffers``).  ``spfh`` uint8 [B,N,36], ``fpfh``
    float32 [B,N,33]; ``normals``: the ``normals.NormalBuffers`` that ``compute_fpfh`` estimates into, whose neighbour lists
    (``idx`` / ``dist``, and with ``search="grid"`` its grid workspace) the descriptor's own search then reuses.  ``error_flag``
    (device int32, cleared at the start of every call that is given these buffers) collects ``_lib.FPFH_ERR_EMPTY`` (a row without a
    single pair: isolated under the radius, or its normal is zero) and ``_lib.FPFH_ERR_NONFINITE`` (a NaN / inf point or normal:
    the pair is skipped, nothing is poisoned)."""

    def __init__(self, N, B, k, device, search="grid"):
        if search not in ("brute", "grid"):
            raise ValueError("features.buffers: search must be \"brute\" or \"grid\"")
        self.B, self.N, self.k, self.search = int(B), int(N), int(k), search
        self.normals = _normals.NormalBuffers(N, B, k, device, cov=False, search=search)
        self.device = self.normals.device
        self.idx, self.dist = self.normals.idx, self.normals.dist
        self.spfh = torch.zeros(B, N, 36, device=device, dtype=torch.uint8)
        self.fpfh = torch.zeros(B, N, 33, device=device, dtype=torch.float32)
        self.error_flag = torch.zeros(1, device=device, dtype=torch.int32)

    def check(self, empty_ok=True):
        """Reads ``error_flag`` back: ``ValueError`` for a point or normal that is not finite, and, unless ``empty_ok`` (an isolated
        point under a radius is ordinary in a scan), for a row without a pair."""
        flag = int(self.error_flag.item())
        if flag & _lib.FPFH_ERR_NONFINITE:
            raise ValueError("fpfh: a point or a normal is not finite; its pairs were skipped")
        if flag & _lib.FPFH_ERR_EMPTY and not empty_ok:
            raise ValueError("fpfh: a row has no pair (no neighbour within the radius, or a zero normal); its own histogram is zero")


def buffers(N, B=1, k=32, device="cuda", search="grid"):
    """Preallocates for ``N`` rows per cloud, ``B`` clouds and up to ``k`` neighbours.  With ``buffers=`` a call allocates nothing,
    reads nothing back and captures into a graph that stays valid when points, normals and the device-side counts change.
    ``search``: which self-search ``compute_fpfh`` will run on them."""
    return FpfhBuffers(N, B, k, device, search)


def _normal_rows(t, B, M, normal_col, flat, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.Pn2Error("%s: normals must live on the GPU: this package has no CPU path" % what)
    if t.dtype != torch.float32 or t.dim() != (2 if flat else 3) or not 3 <= t.shape[-1] <= 16:
        raise RuntimeError("%s: normals must be float32 [M, ld] or [B, M, ld] like the points, 3 <= ld <= 16" % what)
    t = t.contiguous()
    t = t[None] if flat else t
    if t.shape[0] != B or t.shape[1] != M:
        raise ValueError("%s: normals and points disagree on B or M" % what)
    normal_col = int(normal_col)
    if normal_col < 0 or normal_col + 3 > t.shape[2]:
        raise ValueError("%s: columns %d .. %d do not fit a row of %d" % (what, normal_col, normal_col + 2, t.shape[2]))
    return t, normal_col


def _run(what, points, normals, idx, max_dist, normal_col, n_points, err, buf, want_fpfh):
    flat = isinstance(points, torch.Tensor) and points.dim() == 2
    points = _points(points, "points")
    B, M, ldp = points.shape
    dev = points.device
    normals, normal_col = _normal_rows(normals, B, M, normal_col, flat, what)
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise _lib.Pn2Error("%s: idx must live on the GPU: this package has no CPU path" % what)
    if idx.dtype != torch.int64 or idx.dim() != (2 if flat else 3):
        raise ValueError("%s: idx must be an int64 [B, M, K] tensor ([M, K] for [M, ld] points)" % what)
    idx = idx.contiguous()
    idx = idx[None] if flat else idx
    if idx.shape[0] != B or idx.shape[1] != M:
        raise ValueError("%s: idx needs a row per point (the search is a self-search)" % what)
    K = idx.shape[2]
    if K < 1:
        raise RuntimeError("%s: K must be at least 1" % what)
    if K > _lib.KNN_MAX_K:
        raise RuntimeError("%s: K (%d) > %d is not supported (there is no fallback path)" % (what, K, _lib.KNN_MAX_K))
    if buf is not None and (buf.B != B or buf.N != M or buf.device != dev):
        raise ValueError("%s: the buffers were made for B = %d, N = %d on %s" % (what, buf.B, buf.N, buf.device))
    n_points = _counts(n_points, B, dev, "%s: n_points" % what)
    if err is None and buf is not None:
        err = buf.error_flag
        err.zero_()                                              # an async fill, nothing is read back
    if err is not None and (not err.is_cuda or err.dtype != torch.int32 or err.numel() < 1):
        raise ValueError("%s: err must be a device int32 tensor" % what)
    max_d2 = float("inf") if max_dist is None else float(np.float32(float(max_dist) ** 2))
    make = torch.zeros if n_points is not None else torch.empty      # (rows at and beyond the count are not written)
    lib = _lib.load()
    spfh_out = buf.spfh if buf is not None else make((B, M, 36), device=dev, dtype=torch.uint8)
    _lib.check(lib.pn2_spfh(_p(points), ldp, _p(normals), normals.shape[2], normal_col, _p(idx), B, M, K, max_d2, _p(n_points),
                            _p(spfh_out), _p(err), _lib.stream()), "pn2_spfh")
    out = None
    if want_fpfh:
        out = buf.fpfh if buf is not None else make((B, M, 33), device=dev, dtype=torch.float32)
        _lib.check(lib.pn2_fpfh(_p(points), ldp, _p(idx), _p(spfh_out), B, M, K, max_d2, _p(n_points), _p(out), _p(err), _lib.stream()),
                   "pn2_fpfh")
        out = out[0] if flat else out
    return out, (spfh_out[0] if flat else spfh_out)


def spfh(points, normals, idx, max_dist=None, normal_col=0, n_points=None, err=None, buffers=None):
    """The integer half of the descriptor: for every point, how its neighbour pairs fall into 3 x 11 angle bins -> uint8 [B,M,36]
    ([M,36] for [M,ld] points): bytes 0..32 the counts, byte 33 the number of pairs ``m``, bytes 34..35 zero (``spfh_counts``
    unpacks it).  The arguments are ``fpfh``'s."""
    return _run("spfh", points, normals, idx, max_dist, normal_col, n_points, err, buffers, False)[1]


def fpfh(points, normals, idx, max_dist=None, normal_col=0, n_points=None, return_spfh=False, err=None, buffers=None):
    """FPFH descriptors of a cloud from its points, normals and self-search lists -> float32 [B,M,33] ([M,33] for [M,ld] points).

    ``points`` [B,M,ld] (or [M,ld]) float32, 3 <= ld <= 16, columns 0..2 = x, y, z, read where they lie.  ``normals`` float32 of
    the same leading shape with the UNIT normal in columns ``normal_col .. normal_col + 2``; it may be ``points`` itself (a
    ShapeNet-part row ``x y z nx ny nz``: ``normal_col=3``).  ``idx`` int64 [B,M,K], K <= 32, row i = the neighbours of point i, as
    ``knn_point`` or ``GridIndex.query_self`` return it (padding ``idx = M``).  A slot is a pair iff its index is in range, the
    two points differ and lie within ``max_dist`` of each other (None: no cut-off), and both normals are finite and not zero.
    Each pair falls into one of 11 bins for each of three angles between the two normals and the line that joins the points;
    a row's descriptor is its own histogram (in percent) plus the 1 / d^2 weighted mean of its neighbours': each third of a row
    sums to 200.  A row without a pair sets ``FPFH_ERR_EMPTY`` in ``err``, a point or normal that is not finite loses its pairs
    and sets ``FPFH_ERR_NONFINITE``.  ``n_points``: device int64 [B] (or host integers), rows at and beyond it are neither read
    nor written (zeros when the outputs are allocated here).

    THE DESCRIPTOR DEPENDS ON THE SIGN OF THE NORMALS: unoriented normals (PCA's sign is arbitrary) give noisy histograms;
    ``normals.estimate_normals(..., viewpoint=...)`` orients them.

    ``return_spfh``: also the uint8 [.,36] rows of ``spfh``.  ``err``: a zeroed device int32 tensor, nothing is read back here.
    ``buffers``: an ``FpfhBuffers``; the outputs then live there.  The bytes are the same from run to run."""
    out, s = _run("fpfh", points, normals, idx, max_dist, normal_col, n_points, err, buffers, True)
    return (out, s) if return_spfh else out


def compute_fpfh(points, radius, k=32, normals=None, normal_col=0, normal_k=16, normal_radius=None, viewpoint="origin", n_points=None,
                 search="grid", buffers=None):
    """FPFH descriptors of a cloud from its points alone -> float32 [B,M,33] ([M,33] for [M,ld] points).

    Without ``normals`` it estimates them first: ``estimate_normals(points, k=normal_k, radius=normal_radius or radius,
    viewpoint=viewpoint, search=search)`` -- the default ``"origin"`` orients them towards the scanner of a LiDAR scan; the
    descriptor depends on their SIGN (see ``fpfh``).  Then the self-search for the ``k`` nearest within ``radius``:
    ``GridIndex(radius=radius).build(points).query_self(k)`` by default, ``search="brute"``: ``pn2_knn`` with ``min(k, M)`` (the
    cut-off is then applied by the kernels).  Then ``fpfh``.  A [., 4] scan is read where it lies (the brute-force search makes
    one packed xyz copy).  ``n_points``: device int64 [B] (or host integers).  ``buffers``: an ``FpfhBuffers`` made for the same
    ``search``."""
    if search not in ("brute", "grid"):
        raise ValueError("compute_fpfh: search must be \"brute\" or \"grid\"")
    flat = isinstance(points, torch.Tensor) and points.dim() == 2
    pts = _points(points, "points")
    B, M, _ = pts.shape
    dev = pts.device
    k = int(k)
    if k < 1:
        raise RuntimeError("compute_fpfh: k must be at least 1")
    if k > _lib.KNN_MAX_K:
        raise RuntimeError("compute_fpfh: k (%d) > %d is not supported (there is no fallback path)" % (k, _lib.KNN_MAX_K))
    buf = buffers
    if buf is not None and (buf.B != B or buf.N != M or buf.k < k or buf.device != dev or buf.search != search):
        raise ValueError("compute_fpfh: the buffers were made for B = %d, N = %d, k >= %d, search = \"%s\" on %s" %
                         (buf.B, buf.N, buf.k, buf.search, buf.device))
    n_points = _counts(n_points, B, dev, "compute_fpfh: n_points")
    nbuf = None if buf is None else buf.normals
    if normals is None:
        normals = _normals.estimate_normals(pts, k=normal_k, radius=radius if normal_radius is None else normal_radius, viewpoint=viewpoint,
                                            n_points=n_points, buffers=nbuf, search=search)
        normal_col = 0
    elif flat:
        normals = normals[None] if isinstance(normals, torch.Tensor) and normals.dim() == 2 else normals
    if search == "grid":
        gbuf = None if nbuf is None else nbuf.grid
        idx = neighbors.GridIndex(radius=radius).build(pts, n_cand=n_points, buffers=gbuf).query_self(k, buffers=gbuf)
    else:
        kk = min(k, M)
        if nbuf is not None:
            xyz = nbuf.xyz
            xyz.copy_(pts[:, :, :3])
            idx = nbuf.idx.reshape(-1)[:B * M * kk].reshape(B, M, kk)
            dist = nbuf.dist.reshape(-1)[:B * M * kk].reshape(B, M, kk)
        else:
            xyz = pts[:, :, :3].contiguous()
            idx = torch.empty(B, M, kk, device=dev, dtype=torch.int64)      # (rows at and beyond the count are never read)
            dist = torch.empty(B, M, kk, device=dev, dtype=torch.float32)
        _lib.check(_lib.load().pn2_knn(_p(xyz), _p(xyz), B, M, M, kk, _p(n_points), _p(n_points), _p(idx), _p(dist), _lib.stream()),
                   "pn2_knn")
    out = fpfh(pts, normals, idx, max_dist=radius, normal_col=normal_col, n_points=n_points, buffers=buf)
    return out[0] if flat else out


def spfh_counts(spfh):
    """``spfh`` uint8 [..., 36] -> ``(counts int32 [..., 33], m int32 [...])``: the 3 x 11 bin counts and the number of pairs.
    Plain torch."""
    return spfh[..., :33].to(torch.int32), spfh[..., 33].to(torch.int32)


Matches = collections.namedtuple("Matches", "pair_src pair_tgt count idx dist")


def match_workspace_bytes(N, B=1):
    """Bytes of ``pn2_match_pairs``' workspace for ``B`` clouds of up to ``N`` source rows (host-only call)."""
    return _lib.workspace_bytes("pn2_match_pairs_workspace_bytes", (int(B), int(N)), ValueError,
                                "match_features: B = %d clouds of N = %d rows are not supported" % (B, N))


class MatchBuffers:
    """Everything ``match_features`` writes, allocated once (``match_buffers``): ``idx`` int64 / ``dist`` float32 [B,N,2] (the forward
    search), ``back_idx`` / ``back_dist`` [B,M,2] (the search with the roles swapped, with ``mutual``), ``pair_src`` / ``pair_tgt``
    int64 [B,N], ``count`` int64 [B] and the workspace."""

    def __init__(self, N, M, B, device, mutual=True):
        self.N, self.M, self.B, self.mutual = int(N), int(M), int(B), bool(mutual)
        i64 = dict(device=device, dtype=torch.int64)
        self.idx = torch.full((self.B, self.N, 2), self.M, **i64)
        self.device = self.idx.device
        self.dist = torch.full((self.B, self.N, 2), float("inf"), device=device, dtype=torch.float32)
        self.back_idx = torch.full((self.B, self.M, 2), self.N, **i64) if mutual else None
        self.back_dist = torch.full((self.B, self.M, 2), float("inf"), device=device, dtype=torch.float32) if mutual else None
        self.pair_src, self.pair_tgt = torch.full((self.B, self.N), -1, **i64), torch.full((self.B, self.N), -1, **i64)
        self.count = torch.zeros(self.B, **i64)
        self.workspace = torch.empty(match_workspace_bytes(self.N, self.B), device=device, dtype=torch.uint8)


def match_buffers(N, M, B=1, device="cuda", mutual=True):
    """Preallocates for ``B`` pairs of clouds with ``N`` source and ``M`` target rows.  With ``buffers=`` ``match_features`` allocates
    nothing, reads nothing back and captures into a graph that stays valid when the features and the device-side counts change."""
    return MatchBuffers(N, M, B, device, mutual)


def _feature_rows(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.Pn2Error("match_features: %s must live on the GPU: this package has no CPU path" % what)
    if t.dtype != torch.float32 or t.dim() not in (2, 3) or t.shape[-1] < 1 or t.shape[-2] < 1:
        raise RuntimeError("match_features: %s must be float32 [N, D] or [B, N, D]" % what)
    t = t.contiguous()
    return t[None] if t.dim() == 2 else t


def match_features(fs, ft, mutual=True, ratio=0.9, n_source=None, n_target=None, buffers=None):
    """Correspondences between two clouds from their descriptors: for every source row the nearest target row in feature space (an
    exact all-pairs search in float32, equal distances resolved towards the lower index), kept iff it passes the tests.

    ``fs`` [N,D] or [B,N,D], ``ft`` [M,D] or [B,M,D] float32 on the GPU, 1 <= D <= 64 (``compute_fpfh``'s [.,33] rows as they are).
    A row takes part iff its values are all finite and not all zero (the row of an isolated point holds zeros).  ``mutual``: the
    nearest source row of the matched target row must be the row itself (a second search with the roles swapped).  ``ratio`` (None:
    off): the nearest distance must be at most ``ratio`` times the second nearest; the kernel compares the squared distances against
    ``float32(ratio ** 2)``, and a row without a second neighbour passes.  ``n_source`` / ``n_target``: device int64 [B] (or host
    integers), only that many leading rows count.

    Returns ``Matches(pair_src, pair_tgt, count, idx, dist)`` of device tensors: int64 [B,N] source and target row of every kept
    pair in ascending source row, int64 [B] how many (entries at and beyond it are not written: -1 when allocated here), and the
    forward search itself: int64 [B,N,2] (``M``: none) and float32 [B,N,2] squared distances (+inf: none).  [N,D] features drop the
    leading B.  ``buffers``: a ``MatchBuffers``.  The bytes are the same from run to run."""
    flat = isinstance(fs, torch.Tensor) and fs.dim() == 2
    fs, ft = _feature_rows(fs, "fs"), _feature_rows(ft, "ft")
    B, N, D = fs.shape
    M, dev = ft.shape[1], fs.device
    if ft.shape[0] != B or ft.shape[2] != D or ft.device != dev:
        raise ValueError("match_features: fs and ft disagree on B, D or the device")
    if D > _lib.MATCH_MAX_D:
        raise RuntimeError("match_features: D (%d) > %d is not supported (there is no fallback path)" % (D, _lib.MATCH_MAX_D))
    if ratio is None:
        ratio2 = float("inf")
    else:
        if not float(ratio) >= 0.0:
            raise ValueError("match_features: ratio must not be negative")
        ratio2 = float(np.float32(float(ratio) ** 2))
    buf = buffers
    if buf is None:
        buf = MatchBuffers(N, M, B, dev, mutual)
    elif buf.B != B or buf.N != N or buf.M != M or buf.device != dev or (mutual and not buf.mutual):
        raise ValueError("match_features: the buffers were made for B = %d, N = %d, M = %d, mutual = %s on %s" %
                         (buf.B, buf.N, buf.M, buf.mutual, buf.device))
    n_source = _counts(n_source, B, dev, "match_features: n_source")
    n_target = _counts(n_target, B, dev, "match_features: n_target")
    lib, s = _lib.load(), _lib.stream()
    _lib.check(lib.pn2_feature_nn2(_p(fs), D, _p(ft), D, B, N, M, D, _p(n_source), _p(n_target), _p(buf.idx), _p(buf.dist), s), "pn2_feature_nn2")
    back = None
    if mutual:
        back = buf.back_idx
        _lib.check(lib.pn2_feature_nn2(_p(ft), D, _p(fs), D, B, M, N, D, _p(n_target), _p(n_source), _p(back), _p(buf.back_dist), s),
                   "pn2_feature_nn2")
    _lib.check(lib.pn2_match_pairs(_p(buf.idx), _p(buf.dist), _p(back), B, N, M, ratio2, _p(n_source), _p(buf.pair_src), _p(buf.pair_tgt),
                                   _p(buf.count), _p(buf.workspace), s), "pn2_match_pairs")
    res = (buf.pair_src, buf.pair_tgt, buf.count, buf.idx, buf.dist)
    return Matches(*[t[0] if flat else t for t in res])
