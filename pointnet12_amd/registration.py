"""Rigid scan registration: point-to-plane and point-to-point ICP on the grid index (``pn2_icp_step``, csrc/icp.hip; the rule is
stated in include/pn2.h under "ICP step" and in numpy in tests/icp_ref.py).

The reference repository has no registration: like kNN, the voxel grid, clustering, normals and the Lovasz loss this is an
extension.  It is the joint consumer of ``neighbors.GridIndex`` ("the nearest target point within ``max_dist``") and of
``normals.estimate_normals`` (the point-to-plane residual).  One iteration is two launches: a fused transform + search + accumulate
kernel that writes one 29-word partial per 1024 source rows, and a per-cloud kernel that adds the partials in a fixed order, solves
the 6 x 6 system and updates ``[R | t]`` in fp64.  The loop never reads anything back: a cloud that has converged (or turned out
singular) is frozen on the device and its later steps return at once.  OUT OF SCOPE: robust weights, a normal-compatibility test,
multi-resolution, GICP and coloured ICP, a gradient, pose graphs.

ICP only converges from a good ``init``; ``register_global`` produces one from two clouds with an unknown relative pose:
``features.compute_fpfh`` on both, ``features.match_features``, then ``ransac_correspondences`` (``pn2_corr_ransac`` /
``pn2_corr_refit``, csrc/corr_ransac.hip; the rule is stated in include/pn2.h under "correspondence RANSAC" and in numpy in
tests/corr_ransac_ref.py): three-pair hypotheses named by an integer function of the seed, each a closed-form rigid transform,
scored by its count of pairs within ``threshold`` in an all-pairs pass (one hypothesis per lane, the pairs broadcast from LDS), the
best one refitted by Horn's quaternion method on its inliers.  Nothing is read back.  OUT OF SCOPE there: MSAC / LO-RANSAC scores,
an adaptive stopping rule, scale estimation, a gradient, wiring into ``FrameSegmenter``.
"""
import collections

import numpy as np
import torch

from . import _lib, features, neighbors
from . import normals as _normals

_p = _lib.ptr

IcpResult = collections.namedtuple("IcpResult", "transform fitness rmse iterations status corr")
METRICS = {"point": _lib.ICP_POINT, "plane": _lib.ICP_PLANE}
NORMAL_K = 16            # neighbours of the default target normals (estimate_normals(target, k=16, radius=2 * max_dist, search="grid"))


def workspace_bytes(N, B=1):
    """Bytes of ``pn2_icp_step``'s workspace for ``B`` clouds of up to ``N`` source rows (host-only call)."""
    return _lib.workspace_bytes("pn2_icp_workspace_bytes", (int(B), int(N)), ValueError,
                                "icp: B = %d clouds of N = %d rows are not supported" % (B, N))


class IcpBuffers:
    """Everything ``icp`` / ``evaluate`` write, allocated once (``buffers``): the state of the loop (``T`` float64 [B,12], ``sums``
    [B,28], ``count`` int64 [B], ``x`` [B,6], ``status`` / ``iters`` int32 [B]), the results (``transform`` float64 [B,4,4],
    ``fitness`` / ``rmse`` float64 [B], ``corr`` int64 [B,N]), the grid's and the normals' own buffers, and ``error_flag`` (device
    int32, cleared at the start of every call; the steps OR ``_lib.ICP_ERR_*`` into it)."""

    def __init__(self, N, M, B, device, normals=True):
        self.N, self.M, self.B = int(N), int(M), int(B)
        f64 = dict(device=device, dtype=torch.float64)
        self.T = torch.zeros(self.B, 12, **f64)
        self.device = self.T.device
        self.sums, self.x = torch.zeros(self.B, 28, **f64), torch.zeros(self.B, 6, **f64)
        self.count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.status = torch.zeros(self.B, device=device, dtype=torch.int32)
        self.iters = torch.zeros(self.B, device=device, dtype=torch.int32)
        self.corr = torch.full((self.B, self.N), self.M, device=device, dtype=torch.int64)
        self.transform = torch.zeros(self.B, 4, 4, **f64)
        self.transform[:, 3, 3] = 1.0
        self.fitness, self.rmse = torch.zeros(self.B, **f64), torch.zeros(self.B, **f64)
        self.workspace = torch.empty(workspace_bytes(self.N, self.B), device=device, dtype=torch.uint8)
        self.grid = neighbors.GridBuffers(self.M, self.B, 1, 1, device)
        self.normals = _normals.buffers(self.M, B=self.B, k=NORMAL_K, device=device, cov=False, search="grid") if normals else None
        self.error_flag = torch.zeros(1, device=device, dtype=torch.int32)

    def check(self, singular_ok=True):
        """Reads ``error_flag`` back: ``ValueError`` for a source row that is not finite or leaves the grid once transformed, for
        sums or a transform that are not finite, and, unless ``singular_ok`` (``status`` says which clouds), for a singular system."""
        flag = int(self.error_flag.item())
        if flag & _lib.ICP_ERR_NONFINITE:
            raise ValueError("icp: a transform or the normal equations are not finite")
        if flag & _lib.ICP_ERR_QUERY:
            raise ValueError("icp: a transformed source row is not finite or lies outside the grid's 2^21 cells per axis; it took no part")
        if flag & _lib.ICP_ERR_SINGULAR and not singular_ok:
            raise ValueError("icp: the normal equations of a cloud are singular (too few matches, or the matched geometry does not constrain the motion)")


def buffers(N, M, B=1, device="cuda", normals=True):
    """Preallocates for ``B`` pairs of ``N`` source and ``M`` target rows.  With ``buffers=`` a call allocates nothing and reads
    nothing back, and captures into a graph that stays valid when the points, ``init`` and the device-side counts change (``init``
    must then be a device tensor or None).  ``normals=False`` leaves out what the default target normals need."""
    return IcpBuffers(N, M, B, device, normals)


def _pairs(source, target, what):
    flat = isinstance(source, torch.Tensor) and source.dim() == 2
    src, tgt = neighbors._cloud(source, what + ": source"), neighbors._cloud(target, what + ": target")
    if src.shape[0] != tgt.shape[0] or src.device != tgt.device or flat != (isinstance(target, torch.Tensor) and target.dim() == 2):
        raise ValueError("%s: source and target disagree on B, the device or the number of dimensions" % what)
    return flat, src, tgt


def _transforms(init, B, dev, what):
    """None, [3,4], [4,4] or [B,.,4] (tensor or array) -> float64 [B,12] on ``dev`` (a copy)."""
    if init is None:
        return torch.eye(3, 4, device=dev, dtype=torch.float64).reshape(1, 12).repeat(B, 1)
    t = init if isinstance(init, torch.Tensor) else torch.from_numpy(np.asarray(init, np.float64))
    t = t.to(device=dev, dtype=torch.float64)
    if t.dim() == 2:
        t = t[None].expand(B, -1, -1)
    if t.dim() != 3 or t.shape[0] != B or t.shape[1] not in (3, 4) or t.shape[2] != 4:
        raise ValueError("%s: a transform must be [3,4], [4,4] or [B,.,4]" % what)
    return t[:, :3, :].reshape(B, 12).contiguous()


def _setup(source, target, max_dist, index, n_source, n_target, buf, what):
    flat, src, tgt = _pairs(source, target, what)
    B, N, _ = src.shape
    M, dev = tgt.shape[1], src.device
    if not float(max_dist) > 0:
        raise ValueError("%s: max_dist must be positive" % what)
    max_d2 = float(np.float32(float(max_dist) ** 2))
    if buf is not None and (buf.B != B or buf.N != N or buf.M != M or buf.device != dev):
        raise ValueError("%s: the buffers were made for B = %d, N = %d, M = %d on %s" % (what, buf.B, buf.N, buf.M, buf.device))
    n_source = neighbors._counts(n_source, B, dev, what + ": n_source")
    n_target = neighbors._counts(n_target, B, dev, what + ": n_target")
    if index is None:
        index = neighbors.GridIndex(radius=max_dist, device=dev).build(tgt, n_cand=n_target, buffers=None if buf is None else buf.grid)
    else:
        if index._work is None or index._B != B or index._M != M or index._dev != dev:
            raise ValueError("%s: index must be a GridIndex built for the target (B = %d, M = %d)" % (what, B, M))
        if (index.cell < float(np.sqrt(np.float64(max_d2)) * (1.0 + 2.0 ** -20))).any():
            raise ValueError("%s: the index's cells are smaller than max_dist: the search would miss in-range points" % what)
    return flat, src, tgt, B, N, M, dev, max_d2, n_source, n_target, index


def _step(src, tgt, nrm, index, max_d2, metric, flags, tol_rot, tol_trans, n_source, T, sums, count, x, status, iters, corr, err, work):
    B, N, lds = src.shape
    _lib.check(_lib.load().pn2_icp_step(_p(src), lds, B, N, _p(n_source), _p(tgt), tgt.shape[2], tgt.shape[1], _p(nrm),
                                        0 if nrm is None else nrm.shape[2], index._c_origin, index._c_cell, _p(index._work), max_d2,
                                        metric, flags, tol_rot, tol_trans, _p(T), _p(sums), _p(count), _p(x), _p(status), _p(iters),
                                        _p(corr), _p(err), _p(work), _lib.stream()), "pn2_icp_step")


def _score(sums, count, n_source, N, fitness, rmse):
    """fitness = count / n_source, rmse = sqrt(E / count); 0 matches: fitness 0 and rmse +0.0.  Plain torch, nothing read back."""
    n = torch.full_like(count, N) if n_source is None else n_source.clamp(0, N)
    c = count.to(torch.float64)
    some = count > 0
    zero = torch.zeros_like(c)
    torch.where(some, c / n.to(torch.float64).clamp(min=1.0), zero, out=fitness)
    torch.where(some, (sums[:, 27] / c.clamp(min=1.0)).sqrt(), zero, out=rmse)
    return fitness, rmse


def icp(source, target, max_dist, metric="plane", init=None, iterations=30, tol_rot=1e-6, tol_trans=None, target_normals=None, index=None,
        n_source=None, n_target=None, return_corr=False, buffers=None):
    """Registers ``source`` to ``target``: the rigid transform that takes source rows onto the target, by ``iterations`` Gauss-Newton
    steps of ``metric`` ``"plane"`` (point-to-plane, needs target normals) or ``"point"`` (point-to-point), each against the nearest
    target point within ``max_dist`` of the transformed row.

    ``source`` [N,ld] or [B,N,ld], ``target`` [M,ld] or [B,M,ld] float32 on the GPU, 3 <= ld <= 16 (a [.,4] scan is read where it
    lies).  ``init``: [3,4], [4,4] or [B,.,4] (default: the identity).  A cloud stops -- is frozen on the device, its later steps
    cost nothing -- once a step's rotation is at most ``tol_rot`` (radians) and its translation at most ``tol_trans`` (default
    ``1e-6 * max_dist``), or when its normal equations are singular.  ``index``: a ``neighbors.GridIndex`` already built for the
    target (cells at least ``max_dist`` wide); else one is built with ``radius=max_dist``.  ``target_normals`` float32 [.,M,>=3]
    (columns 0..2 are read); for ``"plane"`` they default to ``normals.estimate_normals(target, k=16, radius=2 * max_dist,
    search="grid")``.  ``n_source`` / ``n_target``: device int64 [B] (or host integers), only that many leading rows count.

    Returns ``IcpResult(transform, fitness, rmse, iterations, status, corr)`` of device tensors: float64 [B,4,4]; the share of the
    source rows that have a target point within ``max_dist`` under the result and the root mean square of those distances (one
    more point-metric evaluation; no match: 0 and +0.0); int32 steps taken; int32 ``_lib.ICP_CONVERGED`` / ``_lib.ICP_SINGULAR``
    bits; with ``return_corr`` int64 [B,N] the matched target row (``M``: none), else None.  [N,ld] clouds drop the leading B."""
    what = "icp"
    if metric not in METRICS:
        raise ValueError("icp: metric must be \"plane\" or \"point\"")
    iterations = int(iterations)
    tol_trans = 1e-6 * float(max_dist) if tol_trans is None else float(tol_trans)
    tol_rot = float(tol_rot)
    if iterations < 0 or not (0 <= tol_rot < float("inf")) or not (0 <= tol_trans < float("inf")):
        raise ValueError("icp: iterations and the tolerances must be finite and not negative")
    buf = buffers
    flat, src, tgt, B, N, M, dev, max_d2, n_source, n_target, index = _setup(source, target, max_dist, index, n_source, n_target, buf, what)
    nrm = None
    if metric == "plane":
        if target_normals is None:
            if buf is not None and buf.normals is None:
                raise ValueError("icp: these buffers hold nothing for the default normals (registration.buffers(..., normals=True))")
            nrm = _normals.estimate_normals(tgt, k=NORMAL_K, radius=2.0 * float(max_dist), n_points=n_target, search="grid",
                                            buffers=None if buf is None else buf.normals)
        else:
            nrm = target_normals
            if not isinstance(nrm, torch.Tensor) or nrm.device != dev or nrm.dtype != torch.float32:
                raise ValueError("icp: target_normals must be a float32 tensor on the target's device")
            nrm = (nrm[None] if nrm.dim() == 2 else nrm).contiguous()
            if nrm.dim() != 3 or nrm.shape[0] != B or nrm.shape[1] != M or not 3 <= nrm.shape[2] <= 16:
                raise ValueError("icp: target_normals must be [M, >=3] or [B, M, >=3] like the target")
    if buf is None:
        buf = IcpBuffers(N, M, B, dev, normals=False)
        buf.T.copy_(_transforms(init, B, dev, what))
    else:
        buf.error_flag.zero_()
        buf.status.zero_()
        buf.iters.zero_()
        buf.T.copy_(_transforms(init, B, dev, what))
    for _ in range(iterations):
        _step(src, tgt, nrm, index, max_d2, METRICS[metric], 0, tol_rot, tol_trans, n_source, buf.T, buf.sums, buf.count, buf.x,
              buf.status, buf.iters, None, buf.error_flag, buf.workspace)
    corr = buf.corr if return_corr else None
    _step(src, tgt, None, index, max_d2, _lib.ICP_POINT, _lib.ICP_EVAL_ONLY, 0.0, 0.0, n_source, buf.T, buf.sums, buf.count, None, None,
          None, corr, buf.error_flag, buf.workspace)
    _score(buf.sums, buf.count, n_source, N, buf.fitness, buf.rmse)
    buf.transform[:, :3, :].copy_(buf.T.view(B, 3, 4))
    res = (buf.transform, buf.fitness, buf.rmse, buf.iters, buf.status, corr)
    return IcpResult(*[t[0] if (flat and t is not None) else t for t in res])


def evaluate(source, target, transform, max_dist, index=None, n_source=None, n_target=None, return_corr=False, buffers=None):
    """``icp``'s closing evaluation on its own: ``(fitness, rmse)`` of ``transform`` ([3,4], [4,4] or [B,.,4]) -- the share of the
    source rows with a target point within ``max_dist`` once transformed, and the root mean square of those distances -- followed
    by ``corr`` on request.  Device tensors, float64 [B] (scalars for [N,ld] clouds)."""
    what = "evaluate"
    buf = buffers
    flat, src, tgt, B, N, M, dev, max_d2, n_source, n_target, index = _setup(source, target, max_dist, index, n_source, n_target, buf, what)
    if buf is None:
        buf = IcpBuffers(N, M, B, dev, normals=False)
    else:
        buf.error_flag.zero_()
    buf.T.copy_(_transforms(transform, B, dev, what))
    corr = buf.corr if return_corr else None
    _step(src, tgt, None, index, max_d2, _lib.ICP_POINT, _lib.ICP_EVAL_ONLY, 0.0, 0.0, n_source, buf.T, buf.sums, buf.count, None, None,
          None, corr, buf.error_flag, buf.workspace)
    res = _score(buf.sums, buf.count, n_source, N, buf.fitness, buf.rmse) + ((corr,) if return_corr else ())
    return tuple(t[0] if flat else t for t in res)


def transform_points(points, transform, out=None):
    """``R p + t`` for every row of ``points`` [N,ld] or [B,N,ld] float32 under ``transform`` ([3,4], [4,4] or [B,.,4]), in float64 --
    ``p_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a``, each operation rounded on its own, as ``pn2_icp_step`` transforms a row -- and
    rounded ONCE to float32.  Plain torch (``pn2_point_transform`` is the network's float32 k x k transform).  Returns float32
    [.., N, 3], or ``out`` ([.., N, >=3] float32) with its columns 0..2 written."""
    flat = points.dim() == 2
    pts = points[None] if flat else points
    B = pts.shape[0]
    T = _transforms(transform, B, pts.device, "transform_points").view(B, 3, 4)
    s = pts[:, :, :3].to(torch.float64)
    cols = [((T[:, a, 0, None] * s[:, :, 0] + T[:, a, 1, None] * s[:, :, 1]) + T[:, a, 2, None] * s[:, :, 2]) + T[:, a, 3, None] for a in range(3)]
    res = torch.stack(cols, -1).to(torch.float32)
    res = res[0] if flat else res
    if out is None:
        return res
    out[..., :3] = res
    return out


CorrResult = collections.namedtuple("CorrResult", "transform count rmse best_h status")
GlobalResult = collections.namedtuple("GlobalResult", "transform count rmse best_h status matches")
GLOBAL_THRESHOLD = 0.3   # register_global's default inlier distance as a multiple of the FPFH radius (1.5 voxels against a radius of 5)


def corr_workspace_bytes(N, B=1, iterations=1024):
    """Bytes of ``pn2_corr_ransac`` / ``pn2_corr_refit``'s workspace for ``B`` pair lists of up to ``N`` pairs and ``iterations``
    hypotheses (host-only call)."""
    return _lib.workspace_bytes("pn2_corr_workspace_bytes", (int(B), int(N), int(iterations)), ValueError,
                                "ransac_correspondences: B = %d lists of N = %d pairs with %d hypotheses are not supported" % (B, N, iterations))


class CorrBuffers:
    """Everything ``ransac_correspondences`` writes, allocated once (``corr_buffers``): ``T`` float64 [B,12], ``transform`` float64
    [B,4,4], ``count`` / ``best_count`` int64 [B], ``rmse`` float64 [B], ``sums`` float64 [B,17], ``best_h`` / ``status`` int32 [B],
    ``hyp_count`` int32 [B,iterations], the workspace, and ``error_flag`` (device int32, cleared at the start of every call; the
    launches OR ``_lib.CORR_ERR_*`` into it)."""

    def __init__(self, N, B, iterations, device):
        self.N, self.B, self.H = int(N), int(B), int(iterations)
        f64 = dict(device=device, dtype=torch.float64)
        i32 = dict(device=device, dtype=torch.int32)
        self.T = torch.zeros(self.B, 12, **f64)
        self.device = self.T.device
        self.transform = torch.zeros(self.B, 4, 4, **f64)
        self.transform[:, 3, 3] = 1.0
        self.rmse, self.sums = torch.zeros(self.B, **f64), torch.zeros(self.B, _lib.CORR_SUMS, **f64)
        self.count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.best_count = torch.zeros(self.B, device=device, dtype=torch.int64)
        self.best_h, self.status = torch.zeros(self.B, **i32), torch.zeros(self.B, **i32)
        self.hyp_count = torch.zeros(self.B, self.H, **i32)
        self.workspace = torch.empty(corr_workspace_bytes(self.N, self.B, self.H), device=device, dtype=torch.uint8)
        self.error_flag = torch.zeros(1, **i32)

    def check(self, none_ok=True):
        """Reads ``error_flag`` back: ``ValueError`` for a pair whose rows are out of range or not finite and, unless ``none_ok``
        (``status`` says which clouds), for a cloud in which no transform was found."""
        flag = int(self.error_flag.item())
        if flag & _lib.CORR_ERR_PAIR:
            raise ValueError("ransac_correspondences: a pair names a row outside its cloud; it was never an inlier")
        if flag & _lib.CORR_ERR_NONFINITE:
            raise ValueError("ransac_correspondences: a paired point is not finite; the pair was never an inlier")
        if flag & _lib.CORR_ERR_NONE and not none_ok:
            raise ValueError("ransac_correspondences: a cloud has no valid hypothesis, or its best one has fewer than 3 inliers")


def corr_buffers(N, B=1, iterations=1024, device="cuda"):
    """Preallocates for ``B`` pair lists of up to ``N`` pairs (the source clouds' rows) and ``iterations`` hypotheses.  With
    ``buffers=`` ``ransac_correspondences`` allocates nothing and reads nothing back, and captures into a graph that stays valid when
    the points, the pairs and the device-side count change."""
    return CorrBuffers(N, B, iterations, device)


def ransac_correspondences(source, target, matches, threshold, iterations=1024, seed=0, edge_ratio=0.9, refine=2, buffers=None):
    """The rigid transform that takes the source rows of a pair list onto their target rows, in the presence of wrong pairs:
    ``iterations`` three-pair hypotheses named by an integer function of ``seed``, each scored by its count of pairs that land within
    ``threshold`` of their target row, the best one (the lowest index among equals) refitted ``refine`` times by least squares on its
    inliers (Horn's quaternion method: inliers that lie in a plane are handled, a reflection is never returned).

    ``source`` [N,ld] or [B,N,ld], ``target`` [M,ld] or [B,M,ld] float32 on the GPU, 3 <= ld <= 16.  ``matches``:
    ``features.match_features``' result, or any ``(pair_src, pair_tgt, count)`` of device int64 tensors [B,N], [B,N], [B] (``count``
    may be None: all N).  A hypothesis is dropped unless its three source rows and its three target rows are distinct and every edge
    of the source triangle is as long as the matching target edge to within ``edge_ratio`` (``min >= edge_ratio * max``; 0: off).

    Returns ``CorrResult(transform, count, rmse, best_h, status)`` of device tensors: float64 [B,4,4]; int64 [B] the pairs within
    ``threshold`` under the result and float64 [B] the root mean square of their distances (one closing evaluation); int32 [B] the
    winning hypothesis (-1: none was valid); int32 ``_lib.CORR_NONE`` / ``_lib.CORR_DEGENERATE`` bits.  A cloud with ``CORR_NONE``
    gets the identity, count 0 and rmse 0.  [N,ld] clouds drop the leading B."""
    what = "ransac_correspondences"
    flat, src, tgt = _pairs(source, target, what)
    B, N, _ = src.shape
    M, dev = tgt.shape[1], src.device
    H = int(iterations)
    threshold, edge_ratio = float(threshold), float(edge_ratio)
    if not (np.isfinite(threshold) and threshold >= 0.0) or not 0.0 <= edge_ratio <= 1.0:
        raise ValueError("%s: threshold must be finite and not negative, edge_ratio in [0, 1]" % what)
    if not 1 <= H <= 65536 or int(refine) < 0:
        raise ValueError("%s: iterations must be 1 .. 65536 and refine not negative" % what)
    pair_src, pair_tgt, count = matches[0], matches[1], matches[2]
    for t in (pair_src, pair_tgt):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int64 or t.numel() != B * N or not t.is_contiguous():
            raise ValueError("%s: the pair lists must be contiguous int64 tensors [B, N] = [%d, %d] on the clouds' device" % (what, B, N))
    count = neighbors._counts(count, B, dev, what + ": count")
    buf = buffers
    if buf is None:
        buf = CorrBuffers(N, B, H, dev)
    else:
        if buf.B != B or buf.N != N or buf.H != H or buf.device != dev:
            raise ValueError("%s: the buffers were made for B = %d, N = %d, iterations = %d on %s" % (what, buf.B, buf.N, buf.H, buf.device))
        buf.error_flag.zero_()
    buf.rmse.zero_()
    buf.count.zero_()
    lib, s = _lib.load(), _lib.stream()
    clouds = (_p(src), src.shape[2], _p(tgt), tgt.shape[2], B, N, M, _p(pair_src), _p(pair_tgt), _p(count))
    _lib.check(lib.pn2_corr_ransac(*clouds, H, int(seed) & (2 ** 64 - 1), edge_ratio, threshold, _p(buf.T), None, _p(buf.hyp_count), _p(buf.best_h),
                                   _p(buf.best_count), _p(buf.status), _p(buf.error_flag), _p(buf.workspace), s), "pn2_corr_ransac")
    for flags in [0] * int(refine) + [_lib.CORR_EVAL_ONLY]:
        _lib.check(lib.pn2_corr_refit(*clouds, threshold, flags, _p(buf.T), _p(buf.count), _p(buf.rmse), _p(buf.sums), _p(buf.status),
                                      _p(buf.workspace), s), "pn2_corr_refit")
    buf.transform[:, :3, :].copy_(buf.T.view(B, 3, 4))
    res = (buf.transform, buf.count, buf.rmse, buf.best_h, buf.status)
    return CorrResult(*[t[0] if flat else t for t in res])


class GlobalBuffers:
    """Everything ``register_global`` writes, allocated once (``global_buffers``): ``source_fpfh`` / ``target_fpfh``
    (``features.FpfhBuffers``), ``matches`` (``features.MatchBuffers``) and ``corr`` (``CorrBuffers``, whose ``error_flag`` is
    ``error_flag`` here)."""

    def __init__(self, N, M, B, k, iterations, device, search="grid", mutual=True):
        self.N, self.M, self.B, self.k, self.H, self.search = int(N), int(M), int(B), int(k), int(iterations), search
        self.source_fpfh = features.FpfhBuffers(N, B, k, device, search)
        self.target_fpfh = features.FpfhBuffers(M, B, k, device, search)
        self.matches = features.MatchBuffers(N, M, B, device, mutual)
        self.corr = CorrBuffers(N, B, iterations, device)
        self.device, self.error_flag = self.corr.device, self.corr.error_flag

    def check(self, none_ok=True):
        """Reads the three error flags back: ``FpfhBuffers.check`` of both clouds, then ``CorrBuffers.check``."""
        self.source_fpfh.check()
        self.target_fpfh.check()
        self.corr.check(none_ok)


def global_buffers(N, M, B=1, k=32, iterations=1024, device="cuda", search="grid", mutual=True):
    """Preallocates ``register_global`` for ``B`` pairs of ``N`` source and ``M`` target rows.  With ``buffers=`` the call allocates
    nothing, reads nothing back and captures into a graph that stays valid when the points and the device-side counts change."""
    return GlobalBuffers(N, M, B, k, iterations, device, search, mutual)


def register_global(source, target, radius, threshold=None, k=32, normals=None, search="grid", viewpoint="origin", mutual=True, ratio=0.9,
                    iterations=1024, seed=0, edge_ratio=0.9, refine=2, n_source=None, n_target=None, buffers=None):
    """Registers ``source`` to ``target`` WITHOUT an initial guess: ``features.compute_fpfh(cloud, radius, k)`` on both clouds,
    ``features.match_features(mutual=mutual, ratio=ratio)`` on the descriptors, ``ransac_correspondences(threshold, iterations, seed,
    edge_ratio, refine)`` on the pairs.  The result is meant as ``icp(init=...)``: RANSAC's answer is right to about ``threshold``,
    ICP finishes the job.

    ``source`` [N,ld] or [B,N,ld], ``target`` [M,ld] or [B,M,ld] float32 on the GPU.  ``threshold`` defaults to ``0.3 * radius``
    (``GLOBAL_THRESHOLD``: the usual 1.5 voxels against a descriptor radius of 5 voxels).  ``normals``: a pair ``(source_normals,
    target_normals)`` of float32 tensors with the unit normals in columns 0..2; without it ``compute_fpfh`` estimates them, oriented
    towards ``viewpoint`` (``estimate_normals``' argument, or a pair ``(source_viewpoint, target_viewpoint)``) -- THE DESCRIPTOR
    DEPENDS ON THE SIGN OF THE NORMALS, the default ``"origin"`` suits two scans that are each in their own sensor's frame.  ``search`` is ``compute_fpfh``'s.  ``n_source`` / ``n_target``: device int64 [B] (or host integers).

    Returns ``GlobalResult(transform, count, rmse, best_h, status, matches)``: ``ransac_correspondences``' five and the ``Matches``.
    ``buffers``: a ``GlobalBuffers``; ``buffers.check()`` reads the error flags back."""
    what = "register_global"
    flat, src, tgt = _pairs(source, target, what)
    B, N, _ = src.shape
    M, dev = tgt.shape[1], src.device
    if not float(radius) > 0:
        raise ValueError("register_global: radius must be positive")
    threshold = GLOBAL_THRESHOLD * float(radius) if threshold is None else float(threshold)
    buf = buffers
    if buf is not None and (buf.B != B or buf.N != N or buf.M != M or buf.device != dev or buf.k < int(k) or buf.H != int(iterations) or
                            buf.search != search):
        raise ValueError("register_global: the buffers were made for B = %d, N = %d, M = %d, k >= %d, iterations = %d, search = \"%s\" on %s" %
                         (buf.B, buf.N, buf.M, buf.k, buf.H, buf.search, buf.device))
    ns, nt = (None, None) if normals is None else normals
    if normals is not None and flat:
        ns, nt = ns[None], nt[None]
    vs, vt = viewpoint if isinstance(viewpoint, (tuple, list)) and len(viewpoint) == 2 else (viewpoint, viewpoint)
    n_source = neighbors._counts(n_source, B, dev, what + ": n_source")
    n_target = neighbors._counts(n_target, B, dev, what + ": n_target")
    fs = features.compute_fpfh(src, radius, k=k, normals=ns, viewpoint=vs, n_points=n_source, search=search,
                               buffers=None if buf is None else buf.source_fpfh)
    ft = features.compute_fpfh(tgt, radius, k=k, normals=nt, viewpoint=vt, n_points=n_target, search=search,
                               buffers=None if buf is None else buf.target_fpfh)
    m = features.match_features(fs, ft, mutual=mutual, ratio=ratio, n_source=n_source, n_target=n_target,
                                buffers=None if buf is None else buf.matches)
    r = ransac_correspondences(src, tgt, m, threshold, iterations=iterations, seed=seed, edge_ratio=edge_ratio, refine=refine,
                               buffers=None if buf is None else buf.corr)
    if flat:
        return GlobalResult(r.transform[0], r.count[0], r.rmse[0], r.best_h[0], r.status[0], features.Matches(*[t[0] for t in m]))
    return GlobalResult(*r, m)
