"""The rule of pn2_local_pca (include/pn2.h, "local PCA") in numpy, the inputs the CPU and the GPU test share, and the assertions
both make (tests/test_normals_cpu.py holds the rule to the definition and to its mutants; tests/test_normals_gpu.py holds the
kernel to the rule).

Covariance: IEEE fp64, one pass in ascending slot order, shifted by the first valid slot's point -- numpy's float64 add, multiply
and divide are correctly rounded and nothing here is fused, so `cov` is the statement the kernel must equal bit for bit.
Eigen-solve: np.linalg.eigh (the kernel's method is its own; the bounds below are what it is held to).
"""
import functools

import numpy as np

ERR_FEW, ERR_NONFINITE = 1, 2
QNAN32, QNAN64 = np.uint32(0x7FC00000), np.uint64(0x7FF8000000000000)
SENT_F32, SENT_F64, SENT_I32 = np.float32(-77.25), np.float64(-77.25), np.int32(-7777)

# the bounds of the issue, none fitted to a run
EIG_REL, EIG_ABS_L2, EIG_ABS = 2.0 ** -23, 2.0 ** -45, 2.0 ** -149
UNIT_TOL = 2.0 ** -21            # | |n|^2 - 1 |
RESID_TOL = 2.0 ** -21           # || C n - l0 n ||_inf / l2
NORMAL_TOL = 2.0 ** -23          # per component, on the rows where the reference is well defined
GAP_MIN = 2.0 ** -10             # (l1 - l0) / l2
SIGN_MIN = 2.0 ** -20            # |s| / |v - q|, or |u_z|
ILL_CAP = 0.02                   # at most this share of a case's rows may be ill defined

MUTANTS = ("divisor", "sentinel", "cutoff_ge", "largest", "nosign", "pitch", "lastslot")


def pitched(xyz, ld, fill=np.nan):
    """[..., 3] -> [..., ld] float32 with `fill` (NaN) in the columns no kernel may read."""
    out = np.full(xyz.shape[:-1] + (ld,), fill, np.float32)
    out[..., :3] = xyz
    return out


def covariance(pts, valid, divisor_minus_one=False):
    """pts [R,K,3] float32, valid [R,K] bool -> (cov [R,6] float64, n [R]) by the one-pass rule."""
    R, K, _ = pts.shape
    n = valid.sum(1)
    first = np.where(n > 0, valid.argmax(1), 0)
    p0 = pts[np.arange(R), first].astype(np.float64)
    S1 = np.zeros((R, 3))
    S2 = np.zeros((R, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            v = valid[:, k]
            d = np.where(v[:, None], pts[:, k].astype(np.float64) - p0, 0.0)
            S1 = S1 + d                                          # (+0.0 for a skipped slot: S1 is never -0.0, so this is the identity)
            for j, (a, b) in enumerate(pairs):
                S2[:, j] = S2[:, j] + d[:, a] * d[:, b]
        div = np.maximum(n - 1 if divisor_minus_one else n, 1).astype(np.float64)
        m = S1 / div[:, None]
        C = np.zeros((R, 6))
        for j, (a, b) in enumerate(pairs):
            C[:, j] = S2[:, j] / div - m[:, a] * m[:, b]
    C[n == 0] = 0.0
    return C, n


def full_matrix(C6):
    C = np.empty(C6.shape[:-1] + (3, 3))
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[..., a, b] = C6[..., j]
        C[..., b, a] = C6[..., j]
    return C


def z_rule(u):
    """flip iff u_z < 0; if u_z == 0, iff u_y < 0; if that is 0 too, iff u_x < 0"""
    return (u[:, 2] < 0) | ((u[:, 2] == 0) & ((u[:, 1] < 0) | ((u[:, 1] == 0) & (u[:, 0] < 0))))


def local_pca_ref(cand, idx, dist=None, max_d2=np.inf, query=None, viewpoint=None, n_query=None, expect=None, mutant=None):
    """The rule.  cand [B,M,ldc], idx [B,N,K] int64, dist [B,N,K] or None, query [B,N,ldq] or None, viewpoint [B,3] or None,
    n_query [B] or None, expect: None or [B,N,3] literal unit normals (NaN rows: none) that replace eigh's vector.
    -> dict: normal, eig float32 [B,N,3]; cov float64 [B,N,6]; count int32 [B,N]; err; written, finite, full (n >= 3 and finite),
    well (the reference normal is well defined) bool [B,N]; l float64 [B,N,3] (clamped); u float64 [B,N,3] (signed)."""
    B, M, ldc = cand.shape
    _, N, K = idx.shape
    if mutant == "pitch":
        cand = np.nan_to_num(cand.reshape(B, -1)[:, :M * 3].reshape(B, M, 3), nan=0.5, posinf=0.5, neginf=-0.5)
    if mutant == "lastslot" and K > 1:
        idx, dist, K = idx[..., :K - 1], (None if dist is None else dist[..., :K - 1]), K - 1
    R = B * N
    valid = (idx >= 0) & (idx < M)
    if mutant == "sentinel":
        valid = np.ones_like(valid)
    if dist is not None:
        with np.errstate(invalid="ignore"):
            valid &= ~((dist >= np.float32(max_d2)) if mutant == "cutoff_ge" else (dist > np.float32(max_d2)))
    safe = np.clip(idx, 0, M - 1)
    pts = np.take_along_axis(cand[:, :, None, :3], safe.reshape(B, N * K, 1, 1), axis=1).reshape(R, K, 3)
    valid = valid.reshape(R, K)
    C6, n = covariance(pts, valid, divisor_minus_one=(mutant == "divisor"))
    finite = np.isfinite(np.where(valid[:, :, None], pts, np.float32(0))).all((1, 2))
    w = None
    if viewpoint is not None:
        q = query[:, :, :3].reshape(R, 3)
        finite &= np.isfinite(q).all(1)
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.repeat(viewpoint.astype(np.float64), N, axis=0) - q.astype(np.float64)
    C6f = np.where(finite[:, None], C6, 0.0)
    lam, vec = np.linalg.eigh(full_matrix(C6f))
    l = np.where(lam > 0, lam, 0.0)
    u = vec[:, :, 2 if mutant == "largest" else 0].copy()
    if expect is not None and mutant is None:
        e = expect.reshape(R, 3).astype(np.float64)
        has = ~np.isnan(e).any(1)
        u[has] = e[has]                                          # (already signed: both flips below leave them alone)
    full = finite & (n >= 3)
    well = full & (l[:, 2] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        well &= np.where(l[:, 2] > 0, (l[:, 1] - l[:, 0]) / np.where(l[:, 2] > 0, l[:, 2], 1.0), 0.0) >= GAP_MIN
    if mutant == "nosign":
        big = np.abs(u).argmax(1)
        flip = u[np.arange(R), big] < 0
    elif w is not None:
        wf = np.where(finite[:, None], w, 0.0)
        s = (u[:, 0] * wf[:, 0] + u[:, 1] * wf[:, 1]) + u[:, 2] * wf[:, 2]
        flip = np.where(s == 0, z_rule(u), s < 0)
        well &= np.abs(s) >= SIGN_MIN * np.sqrt((wf * wf).sum(1))
    else:
        flip = z_rule(u)
        well &= np.abs(u[:, 2]) >= SIGN_MIN
    if expect is not None and mutant is None:
        flip[has] = False
        well[has & full] = True                                  # literal normals are never left out
    u = np.where(flip[:, None], -u, u)
    normal = np.where(full[:, None], u, 0.0).astype(np.float32)
    eig = l.astype(np.float32)
    cov = C6.copy()
    normal.view(np.uint32)[~finite] = QNAN32
    eig.view(np.uint32)[~finite] = QNAN32
    cov.view(np.uint64)[~finite] = QNAN64
    nq = np.full(B, N, np.int64) if n_query is None else np.clip(np.asarray(n_query, np.int64), 0, N)
    written = (np.arange(N)[None, :] < nq[:, None])
    wr = written.reshape(R)
    err = (ERR_FEW if (wr & finite & (n < 3)).any() else 0) | (ERR_NONFINITE if (wr & ~finite).any() else 0)
    sh = lambda a, *t: a.reshape((B, N) + t)
    return dict(normal=sh(normal, 3), eig=sh(eig, 3), cov=sh(cov, 6), count=sh(n.astype(np.int32)), err=err, written=written,
                finite=sh(finite), full=sh(full), well=sh(well), l=sh(l, 3), u=sh(u, 3))


def sentinel_outputs(B, N, ldn):
    return dict(normal=np.full((B, N, ldn), SENT_F32, np.float32), eig=np.full((B, N, 3), SENT_F32, np.float32),
                cov=np.full((B, N, 6), SENT_F64, np.float64), count=np.full((B, N), SENT_I32, np.int32), err=0)


def outputs_of(ref, ldn):
    """What a kernel that follows `ref` leaves in sentinel-filled buffers."""
    B, N = ref["count"].shape
    out = sentinel_outputs(B, N, ldn)
    w = ref["written"]
    out["normal"][..., :3][w] = ref["normal"][w]
    for key in ("eig", "cov", "count"):
        out[key][w] = ref[key][w]
    out["err"] = ref["err"]
    return out


def check_outputs(case, ref, got):
    """Every assertion the GPU test makes on a case's outputs (`got`: the sentinel-filled buffers after the call).
    -> the largest measured error per output in units of its bound."""
    w, fin, full = ref["written"], ref["finite"], ref["full"]
    name = case["name"]
    nb = got["normal"]
    assert (nb[..., 3:].view(np.uint32) == SENT_F32.view(np.uint32)).all(), name + ": a column beside the normal was written"
    assert (nb[~w].view(np.uint32) == SENT_F32.view(np.uint32)).all() and (got["eig"][~w] == SENT_F32).all() and \
        (got["cov"][~w] == SENT_F64).all() and (got["count"][~w] == SENT_I32).all(), name + ": a row beyond n_query was written"
    normal = nb[..., :3]
    assert (got["count"][w] == ref["count"][w]).all(), name + ": count"
    bad = np.argwhere(got["cov"][w].view(np.uint64) != ref["cov"][w].view(np.uint64))
    assert len(bad) == 0, (name, "cov bits", len(bad), bad[:4])
    assert got["err"] == ref["err"], (name, "err", got["err"], ref["err"])
    nf = w & ~fin
    assert (normal[nf].view(np.uint32) == QNAN32).all() and (got["eig"][nf].view(np.uint32) == QNAN32).all(), name + ": NaN pattern"
    few = w & fin & ~full
    assert (normal[few].view(np.uint32) == 0).all(), name + ": a row with n < 3 must hold three +0.0"
    rec = dict(eig=0.0, unit=0.0, resid=0.0, normal=0.0, ill=0.0)
    m = w & fin
    if m.any():
        lo, lr = got["eig"][m].astype(np.float64), ref["l"][m]
        bound = EIG_REL * np.abs(lr) + EIG_ABS_L2 * lr[:, 2:3] + EIG_ABS
        r = np.abs(lo - lr) / bound
        assert (r <= 1).all(), (name, "eigenvalue", float(r.max()))
        assert np.isfinite(lo).all() and (np.signbit(lo) == 0).all(), name + ": an eigenvalue below zero or -0.0"
        rec["eig"] = float(r.max())
    m = w & full
    if m.any():
        nn = normal[m].astype(np.float64)
        unit = np.abs((nn * nn).sum(1) - 1.0)
        assert (unit <= UNIT_TOL).all(), (name, "unit", float(unit.max()))
        C = full_matrix(ref["cov"][m])
        l0, l2 = ref["l"][m][:, 0], ref["l"][m][:, 2]
        res = np.abs(np.einsum("rab,rb->ra", C, nn) - l0[:, None] * nn).max(1)
        assert (res <= RESID_TOL * l2).all(), (name, "residual", float((res / np.where(l2 > 0, l2, 1)).max()))
        rec["unit"] = float(unit.max() / UNIT_TOL)
        rec["resid"] = float((res[l2 > 0] / (RESID_TOL * l2[l2 > 0])).max()) if (l2 > 0).any() else 0.0
    ill = m & ~ref["well"]
    rec["ill"] = float(ill.sum()) / max(1, int(w.sum()))
    assert ill.sum() <= ILL_CAP * w.sum(), (name, "rows without a well-defined reference normal", int(ill.sum()), int(w.sum()))
    mw = m & ref["well"]
    if mw.any():
        dn = np.abs(normal[mw].astype(np.float64) - ref["normal"][mw].astype(np.float64)).max(1)
        assert (dn <= NORMAL_TOL).all(), (name, "normal", float(dn.max()), int((dn > NORMAL_TOL).sum()))
        rec["normal"] = float(dn.max() / NORMAL_TOL)
    return rec


# ------------------------------------------------------------------------------------------------------------------ inputs

def knn_np(q, c, K):
    """[B,N,3], [B,M,3] float32 -> idx int64 [B,N,K], float32 squared distances: fp64 distances, a stable sort, pn2_knn's
    sentinel (idx = M, dist = +inf) in the slots beyond M."""
    B, N, _ = q.shape
    M = c.shape[1]
    d = ((q[:, :, None, :].astype(np.float64) - c[:, None, :, :].astype(np.float64)) ** 2).sum(-1)
    order = np.argsort(d, axis=-1, kind="stable")[..., :K]
    idx = np.full((B, N, K), M, np.int64)
    dist = np.full((B, N, K), np.inf, np.float32)
    idx[..., :order.shape[-1]] = order
    dist[..., :order.shape[-1]] = np.take_along_axis(d, order, -1).astype(np.float32)
    return idx, dist


def _case(name, cand, idx, ldc=3, ldq=3, ldn=3, dist=None, max_d2=np.inf, query=None, viewpoint=None, n_query=None, expect=None):
    B, N, K = idx.shape
    return dict(name=name, B=B, N=N, M=cand.shape[1], K=K, ldc=ldc, ldq=ldq, ldn=ldn, cand=pitched(cand, ldc), idx=idx, dist=dist,
                max_d2=float(np.float32(max_d2)), query=None if query is None else pitched(query, ldq),
                viewpoint=None if viewpoint is None else np.asarray(viewpoint, np.float32).reshape(B, 3),
                n_query=None if n_query is None else np.asarray(n_query, np.int64), expect=expect)


def cloud_case(N, K, B=1, M=None, ldc=3, ldq=3, ldn=3, self_query=True, cut=False, viewpoint=False, n_query=None, seed=0):
    """A uniform cloud and its k nearest neighbours (the query is one of its own neighbours in a self-search)."""
    rng = np.random.default_rng(1000 * N + 10 * K + B + seed)
    M = M or max(N, K + 8)
    c = rng.random((B, M, 3), np.float32)
    q = c[:, :N].copy() if self_query else rng.random((B, N, 3), np.float32)
    idx, dist = knn_np(q, c, K)
    max_d2 = np.inf
    if cut:
        max_d2 = np.float32(np.median(dist[..., K // 2]))       # about half the rows lose their far half
        r = rng.integers(0, N, 2)
        dist[0, r[0], K - 1] = max_d2                            # exactly at the cut-off: kept
        dist[0, r[1], K - 1] = np.nextafter(max_d2, np.float32(np.inf))      # the next float above: dropped
    vp = rng.random((B, 3)).astype(np.float32) * 4 - 2 if viewpoint else None
    name = "cloud N=%d K=%d B=%d ld=%d/%d/%d%s%s%s" % (N, K, B, ldc, ldq, ldn, " cut" if cut else "", " vp" if viewpoint else "",
                                                       "" if n_query is None else " nq=%s" % (list(n_query),))
    return _case(name, c, idx, ldc, ldq, ldn, dist if cut or seed % 2 == 0 else None, max_d2, q if (viewpoint or not self_query) else None,
                 vp, n_query)


def planted_case(seed=0, viewpoint=False):
    """Random neighbour lists with planted sentinels (M, -1, far outside), repeats, a slot exactly at the cut-off and one just above."""
    rng = np.random.default_rng(77 + seed)
    B, N, M, K = 3, 257, 300, 9
    c = rng.random((B, M, 3), np.float32)
    q = rng.random((B, N, 3), np.float32)
    idx = rng.integers(0, M, (B, N, K)).astype(np.int64)
    idx[:, ::3, 2] = M                                           # pn2_knn's empty slot
    idx[:, 1::5, 0] = -1                                         # the FIRST slot invalid: p0 is a later one
    idx[:, 2::7, K - 1] = 1 << 40
    idx[:, ::4, 5] = idx[:, ::4, 4]                              # repeats count once per appearance
    idx[0, 10, :] = M                                            # n = 0
    idx[0, 12, 2:] = M                                           # n = 2
    idx[1, 13, :] = 7                                            # one point K times: C = 0 with n = K
    dist = rng.random((B, N, K), np.float32)
    max_d2 = np.float32(0.75)
    dist[:, ::2, 3] = max_d2                                     # kept
    dist[:, 1::2, 3] = np.nextafter(max_d2, np.float32(np.inf))  # dropped
    idx[0, 11, :] = -1
    idx[0, 11, 4] = 3                                            # n = 1: one valid slot, not the first
    dist[0, 11, 4] = 0.125
    dist[0, 12, :2] = 0.125                                      # (row 12's two slots are inside the cut-off)
    dist[2, 5, :] = np.nan                                       # !(NaN > max_d2): kept
    vp = np.float32([[2, 2, 2], [-1, 0.5, 0.5], [0.5, 0.5, 9]]) if viewpoint else None
    return _case("planted%s" % (" vp" if viewpoint else ""), c, idx, 4, 7, 7, dist, max_d2, q if viewpoint else None, vp, [257, 100, 64])


def nonfinite_case(viewpoint=False):
    """A NaN and an inf candidate: the rows that use them hold the NaN patterns, rows whose bad slot is cut off or a sentinel
    do not; with a viewpoint, a query that is not finite does the same."""
    rng = np.random.default_rng(5)
    B, N, M, K = 1, 130, 64, 6
    c = rng.random((B, M, 3), np.float32)
    c[0, 3, 1] = np.nan
    c[0, 9, 0] = np.inf
    c[0, 11, 2] = -np.inf
    q = rng.random((B, N, 3), np.float32)
    idx = rng.integers(12, M, (B, N, K)).astype(np.int64)
    dist = np.full((B, N, K), 0.25, np.float32)
    idx[0, 0, 2] = 3
    idx[0, 1, 0] = 9
    idx[0, 64, 5] = 11
    idx[0, 2, 4] = 3
    dist[0, 2, 4] = 2.0                                          # the NaN candidate is cut off: the row is finite
    idx[0, 3, :] = [3, 9, 11, 64, -1, 64]                        # n = 3, all three bad
    idx[0, 4, :] = [3, 64, 64, 64, 64, 64]                       # n = 1 and not finite: NONFINITE, not FEW
    if viewpoint:
        q[0, 100, 1] = np.nan                                    # a query that is not finite matters only with a viewpoint
    return _case("nonfinite%s" % (" vp" if viewpoint else ""), c, idx, 4, 4, 6, dist, 1.0, q, [[0.5, 0.5, 3]] if viewpoint else None)


def _patch_idx(G):
    """The 3 x 3 patch (clamped at the border) around every node of a G x G grid -> [G * G, 9]."""
    a = np.clip(np.arange(G), 1, G - 2)                          # the patch's centre: a border node takes its inner neighbour's patch
    ci, cj = np.meshgrid(a, a, indexing="ij")
    out = [((ci + di) * G + (cj + dj)).reshape(-1) for di in (-1, 0, 1) for dj in (-1, 0, 1)]
    return np.stack(out, 1).astype(np.int64)


def plane_case(axis, viewpoint=None):
    """An exact lattice plane (coordinates on a grid of 1/8, the normal along `axis`): every 3 x 3 patch gives the axis exactly."""
    G = 9
    a = np.arange(G, dtype=np.float32) / 8
    u, v = np.meshgrid(a, a, indexing="ij")
    pts = np.empty((1, G * G, 3), np.float32)
    others = [x for x in range(3) if x != axis]
    pts[0, :, others[0]] = u.reshape(-1) - 0.5
    pts[0, :, others[1]] = v.reshape(-1) * 2 + 0.25
    pts[0, :, axis] = 0.375
    idx = _patch_idx(G)[None]
    expect = np.zeros((1, G * G, 3))
    expect[..., axis] = 1.0
    vp = None
    if viewpoint is not None:
        vp = np.zeros((1, 3), np.float32)
        vp[0, axis] = viewpoint                                  # above (+) or below (-) the plane
        if viewpoint < 0.375:
            expect = -expect
    return _case("plane axis=%d vp=%s" % (axis, viewpoint), pts, idx, 4, 4, 6, None, np.inf, pts if vp is not None else None, vp,
                 None, expect)


def line_case(axis):
    """An exact lattice line along `axis`: C is diagonal with one entry, the kernel's rule gives the lowest OTHER axis."""
    M = 70
    pts = np.zeros((1, M, 3), np.float32)
    pts[0, :, axis] = np.arange(M, dtype=np.float32) / 4 - 3
    pts[0, :, (axis + 1) % 3] = 1.5
    idx = np.clip(np.arange(M)[:, None] + np.arange(-2, 3)[None, :], 0, M - 1).astype(np.int64)[None]
    expect = np.zeros((1, M, 3))
    expect[..., 1 if axis == 0 else 0] = 1.0
    return _case("line axis=%d" % axis, pts, idx, 3, 3, 3, None, np.inf, None, None, None, expect)


def equal_case():
    """All points equal: C = 0 with n = K >= 3, the rule gives +x."""
    pts = np.full((1, 65, 3), 0.625, np.float32)
    idx = np.random.default_rng(3).integers(0, 65, (1, 65, 4)).astype(np.int64)
    expect = np.zeros((1, 65, 3))
    expect[..., 0] = 1.0
    return _case("all equal", pts, idx, 3, 3, 3, None, np.inf, None, None, None, expect)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case of the two tests.  N: 1, 63, 64, 65, 255, 256, 257, 1000.  K: 1, 2, 3, 4, 7, 8, 9, 16, 31, 32, 33, 64.  B: 1, 3 with
    ragged n_query including 0.  ldc / ldq: 3, 4, 7.  ldn: 3, 6, 7."""
    cs = [
        cloud_case(1, 3, M=40),
        cloud_case(63, 1, ldc=4, seed=1),
        cloud_case(64, 2, B=3, n_query=[64, 0, 17]),
        cloud_case(65, 4, ldc=7, ldq=4, ldn=6, viewpoint=True, self_query=False, M=90),
        cloud_case(255, 3, ldc=4, ldq=4, cut=False, seed=1),
        cloud_case(255, 7, ldn=7, cut=True),
        cloud_case(256, 8, B=3, n_query=[256, 100, 0], viewpoint=True, ldq=7),
        cloud_case(257, 9, ldc=4, ldq=4, cut=True, viewpoint=True),
        cloud_case(1000, 16, ldc=4, ldq=4, ldn=6, viewpoint=True, cut=True),
        cloud_case(257, 31, seed=1),
        cloud_case(65, 32, cut=True),
        cloud_case(64, 33, M=200, self_query=False),
        cloud_case(63, 64, B=3, M=300, ldc=7, n_query=[5, 63, 40]),
        cloud_case(20, 16, M=10, self_query=False),              # K > M: pn2_knn's empty slots
        planted_case(), planted_case(viewpoint=True), nonfinite_case(), nonfinite_case(viewpoint=True),
        plane_case(0), plane_case(1), plane_case(2), plane_case(2, viewpoint=5.0), plane_case(2, viewpoint=-5.0), plane_case(0, viewpoint=-1.0),
        line_case(0), line_case(1), line_case(2), equal_case(),
    ]
    for c in cs:
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def reference(i, mutant=None):
    c = cases()[i]
    return local_pca_ref(c["cand"], c["idx"], c["dist"], c["max_d2"], c["query"], c["viewpoint"], c["n_query"], c["expect"], mutant)


# ------------------------------------------------------------------------------------------------------------------ solver

def jacobi_eig3(C6, sweeps):
    """The kernel's solver restated (csrc/sym_eig3.h): cyclic Jacobi, a fixed number of sweeps, rotations (0,1), (0,2), (1,2).
    C6 [R,6] -> (diag [R,3] unsorted, V [R,3,3] columns, off [sweeps,R]: the off-diagonal norm after each sweep)."""
    A = full_matrix(np.asarray(C6, np.float64)).copy()
    R = A.shape[0]
    V = np.tile(np.eye(3), (R, 1, 1))
    off = []
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = A[:, p, q].copy()
                on = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0, -t, t)
                t = np.where(on, t, 0.0)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * np.where(on, apq, 0.0)
                A[:, p, p] = np.where(on, A[:, p, p] - h, A[:, p, p])
                A[:, q, q] = np.where(on, A[:, q, q] + h, A[:, q, q])
                A[:, p, q] = A[:, q, p] = 0.0
                rp, rq = A[:, r, p].copy(), A[:, r, q].copy()
                A[:, r, p] = A[:, p, r] = np.where(on, c * rp - s * rq, rp)
                A[:, r, q] = A[:, q, r] = np.where(on, s * rp + c * rq, rq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(on[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(on[:, None], s[:, None] * vp + c[:, None] * vq, vq)
            off.append(np.sqrt(A[:, 0, 1] ** 2 + A[:, 0, 2] ** 2 + A[:, 1, 2] ** 2))
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), V, np.stack(off)
