"""The matching rule of include/pn2.h ("feature matching") in numpy: what pn2_feature_nn2 and pn2_match_pairs must write.

The distance is float32 arithmetic in a Python loop over the column c: ``t = q[c] - f[c]; s = s + t * t``, one rounding per operation
(numpy never fuses), over all [N,M] pairs at once.  The two nearest are taken by a stable argsort of the distances (equal distances
keep their index order: the strict compares of the kernel), NaN and +inf never kept."""
import numpy as np


def takes_part(f, D):
    """bool [rows]: the D values are all finite and not all zero."""
    f = np.asarray(f, np.float32)[:, :D]
    return np.isfinite(f).all(1) & (f != 0).any(1)


def dist2(q, f, D):
    """float32 [N,M]: the header's d2 for every pair of rows."""
    q, f = np.asarray(q, np.float32), np.asarray(f, np.float32)
    s = np.zeros((q.shape[0], f.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for c in range(D):
            t = q[:, c, None] - f[None, :, c]
            s = s + t * t
    return s


def nn2_cloud(q, f, D, nq, mc, idx, dist):
    """One cloud: writes rows < nq of idx int64 [N,2] / dist float32 [N,2] in place."""
    M = f.shape[0]
    if nq == 0:
        return
    d = dist2(q[:nq], f[:mc], D)
    ok_q, ok_f = takes_part(q[:nq], D), takes_part(f[:mc], D)
    d = np.where(ok_q[:, None] & ok_f[None, :] & np.isfinite(d), d, np.float32(np.inf))
    d = np.concatenate([d, np.full((nq, 2), np.inf, np.float32)], 1)          # (two "none" columns: an argsort always finds two)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    best = np.take_along_axis(d, order, 1)
    idx[:nq] = np.where(np.isfinite(best), order, M)
    dist[:nq] = best


def feature_nn2(query, cand, D, n_query=None, n_cand=None, idx_before=None, dist_before=None):
    """pn2_feature_nn2 on numpy inputs [B,N,ldq] / [B,M,ldc] -> (idx int64 [B,N,2], dist float32 [B,N,2]); rows at and beyond
    n_query keep ``*_before`` (default: M and +inf)."""
    query, cand = np.asarray(query, np.float32), np.asarray(cand, np.float32)
    B, N, M = query.shape[0], query.shape[1], cand.shape[1]
    idx = np.full((B, N, 2), M, np.int64) if idx_before is None else np.array(idx_before, np.int64)
    dist = np.full((B, N, 2), np.inf, np.float32) if dist_before is None else np.array(dist_before, np.float32)
    nq = np.full(B, N) if n_query is None else np.clip(np.asarray(n_query, np.int64), 0, N)
    mc = np.full(B, M) if n_cand is None else np.clip(np.asarray(n_cand, np.int64), 0, M)
    for b in range(B):
        nn2_cloud(query[b], cand[b], D, int(nq[b]), int(mc[b]), idx[b], dist[b])
    return idx, dist


def keep_rows(idx_b, dist_b, back_b, M, ratio2, nq):
    """bool [nq]: the rows of one cloud that pn2_match_pairs keeps."""
    j = idx_b[:nq, 0]
    keep = (j >= 0) & (j < M)
    if back_b is not None:
        keep &= back_b[np.clip(j, 0, M - 1), 0] == np.arange(nq)
    a, c = dist_b[:nq, 0].astype(np.float32), dist_b[:nq, 1].astype(np.float32)
    with np.errstate(all="ignore"):
        ratio = np.ones(nq, bool) if np.isposinf(ratio2) else (np.isposinf(c) | (a <= np.float32(ratio2) * c))
    return keep & ratio


def match_pairs(idx, dist, back, M, ratio2, n_query=None, fill=-1):
    """pn2_match_pairs on numpy inputs -> (pair_src int64 [B,N], pair_tgt int64 [B,N], count int64 [B]); entries at and beyond
    count hold ``fill``."""
    B, N = idx.shape[:2]
    nq = np.full(B, N) if n_query is None else np.clip(np.asarray(n_query, np.int64), 0, N)
    src, tgt, count = np.full((B, N), fill, np.int64), np.full((B, N), fill, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        keep = np.flatnonzero(keep_rows(idx[b], dist[b], None if back is None else back[b], M, ratio2, int(nq[b])))
        count[b] = len(keep)
        src[b, :len(keep)], tgt[b, :len(keep)] = keep, idx[b, keep, 0]
    return src, tgt, count


def match_features(fs, ft, D, mutual=True, ratio=0.9, n_source=None, n_target=None):
    """The whole matcher on numpy inputs: forward search, backward search when ``mutual``, the filter with ratio2 = float32(ratio^2)."""
    idx, dist = feature_nn2(fs, ft, D, n_source, n_target)
    back = feature_nn2(ft, fs, D, n_target, n_source)[0] if mutual else None
    ratio2 = np.inf if ratio is None else float(np.float32(float(ratio) ** 2))
    return match_pairs(idx, dist, back, ft.shape[1], ratio2, n_source) + (idx, dist)
