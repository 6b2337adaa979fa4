"""GPU: pn2_local_pca (csrc/normals.hip) and pointnet12_amd.normals against the numpy rule of tests/normals_ref.py.

Every case goes through the C ABI into sentinel-filled buffers with guard words behind them; the assertions are
normals_ref.check_outputs -- the ones tests/test_normals_cpu.py makes on the rule itself and on its mutants:
    cov, count: bit for bit;  err, the NaN patterns, the +0.0 normals of rows with n < 3: exact;
    eigenvalues: |out - l| <= 2^-23 |l| + 2^-45 l2 + 2^-149;
    every finite row with n >= 3: | |n|^2 - 1 | <= 2^-21 and || C n - l0 n ||_inf <= 2^-21 l2;
    the normal against the reference's, 2^-23 per component, where the reference is well defined (at most 2 % of a case's rows
    are not; the lattice planes and lines, with literal normals, always are).
What the shapes are for (local_pca_kernel: 256 rows per workgroup, one per lane, slots in groups of four with a scalar tail):
    N 1, 63, 64, 65, 255, 256, 257, 1000: wave and workgroup edges;  K 1 .. 64: no group, one, tails of 1 .. 3, many groups;
    B 1, 3 with ragged n_query including 0;  ldc / ldq 3, 4, 7 and ldn 3, 6, 7 with NaN in the columns no kernel may read.

The largest measured errors in units of their bounds are printed (run with -s); README.md records one run.
"""
import numpy as np
import pytest
import torch

import normals_ref as NR
from pointnet12_amd import _lib
from pointnet12_amd import normals as PN
from pointnet12_amd import pointnet_util as U

pytestmark = pytest.mark.gpu

CASES = NR.cases()
IDS = [c["name"] for c in CASES]
GUARD = 64
EINVAL = -1


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)     # (a copy: the cached arrays are read-only)


def run_raw(dev, case, want=("normal", "eig", "cov", "count", "err"), override=None):
    """pn2_local_pca through the C ABI -> (rc, outputs as numpy, guards intact)."""
    a = dict(case)
    a.update(override or {})
    B, N, M, K, ldn = a["B"], a["N"], a["M"], a["K"], a["ldn"]
    s = NR.sentinel_outputs(B, N, ldn)
    bufs = {k: torch.cat([cu(s[k].reshape(-1), dev), cu(np.full(GUARD, s[k].reshape(-1)[0]), dev)]) for k in ("normal", "eig", "cov", "count")}
    err = torch.zeros(1 + GUARD, device=dev, dtype=torch.int32)
    cand, query, idx, dist = cu(a["cand"], dev), cu(a["query"], dev), cu(a["idx"], dev), cu(a["dist"], dev)
    nq, vp = cu(a["n_query"], dev), cu(a["viewpoint"], dev)
    p = _lib.ptr
    g = lambda k: p(bufs[k]) if k in want else None
    rc = _lib.load().pn2_local_pca(p(query), a["ldq"], p(cand), a["ldc"], p(idx), p(dist), B, N, M, K, a["max_d2"], p(nq), p(vp),
                                   g("normal"), ldn, g("eig"), g("cov"), g("count"), p(err) if "err" in want else None, _lib.stream())
    torch.cuda.synchronize()
    out, guards = {}, True
    for k, shape in (("normal", (B, N, ldn)), ("eig", (B, N, 3)), ("cov", (B, N, 6)), ("count", (B, N))):
        h = bufs[k].cpu().numpy()
        out[k] = h[:-GUARD].reshape(shape)
        guards = guards and (h[-GUARD:] == s[k].reshape(-1)[0]).all()
    e = err.cpu().numpy()
    out["err"] = int(e[0])
    return rc, out, bool(guards and (e[1:] == 0).all())


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_local_pca_vs_rule(dev, i):
    case, ref = CASES[i], NR.reference(i)
    rc, out, guards = run_raw(dev, case)
    assert rc == 0 and guards
    rec = NR.check_outputs(case, ref, out)
    print("\n%s: largest error / bound: eig %.3f  unit %.3f  residual %.3f  normal %.3f  (ill-defined rows %.2f %%)"
          % (case["name"], rec["eig"], rec["unit"], rec["resid"], rec["normal"], 100 * rec["ill"]))
    rc2, out2, guards2 = run_raw(dev, case)
    assert rc2 == 0 and guards2 and same_bytes(out, out2), "two runs differ"


@pytest.mark.parametrize("want", [(), ("normal",), ("eig", "err"), ("cov", "count")])
def test_every_output_may_be_null(dev, want):
    i = IDS.index("planted vp")
    case, ref = CASES[i], NR.reference(i)
    rc, out, guards = run_raw(dev, case, want=want)
    assert rc == 0 and guards
    full = NR.outputs_of(ref, case["ldn"])
    blank = NR.sentinel_outputs(case["B"], case["N"], case["ldn"])
    rc_all, out_all, _ = run_raw(dev, case)
    for k in ("normal", "eig", "cov", "count"):
        expect = out_all[k] if k in want else blank[k]
        assert np.array_equal(out[k].view(np.uint8), expect.view(np.uint8)), k
    assert out["err"] == (full["err"] if "err" in want else 0)


def test_idx_from_pn2_knn(dev):
    """The neighbour lists as pn2_knn writes them (K = 16 of 1000 and, with K > n_cand, its empty slots idx = M, dist = +inf), a
    radius as the cut-off, a [., 4] cloud read where it lies."""
    rng = np.random.default_rng(11)
    B, M, K = 2, 1000, 16
    xyz = rng.random((B, M, 3), np.float32)
    xyz[1, :9] = np.float32(0.5) + xyz[1, :9] / 20               # (within the radius of one another)
    n = np.int64([1000, 9])                                      # cloud 1: nine candidates for sixteen slots
    xd, nd = cu(xyz, dev), cu(n, dev)
    idx = torch.full((B, M, K), -5, device=dev, dtype=torch.int64)
    dist = torch.full((B, M, K), -5.0, device=dev, dtype=torch.float32)
    p = _lib.ptr
    assert _lib.load().pn2_knn(p(xd), p(xd), B, M, M, K, p(nd), p(nd), p(idx), p(dist), _lib.stream()) == 0
    torch.cuda.synchronize()
    ih, dh = idx.cpu().numpy(), dist.cpu().numpy()
    assert (ih[1, :9, 9:] == M).all() and np.isinf(dh[1, :9, 9:]).all()
    case = NR._case("from pn2_knn", xyz, ih, 4, 4, 6, dh, np.float32(0.12) ** 2, xyz, [[0.5, 0.5, 4.0], [9.0, 0.5, 0.5]], n)
    ref = NR.local_pca_ref(case["cand"], case["idx"], case["dist"], case["max_d2"], case["query"], case["viewpoint"], case["n_query"])
    rc, out, guards = run_raw(dev, case)
    assert rc == 0 and guards
    rec = NR.check_outputs(case, ref, out)
    assert (ref["count"][0] >= 1).all() and (ref["count"][0] < K).any() and (ref["count"][1, :9] == 9).all()
    print("\nfrom pn2_knn: largest error / bound: eig %.3f  unit %.3f  residual %.3f  normal %.3f  (ill-defined rows %.2f %%)"
          % (rec["eig"], rec["unit"], rec["resid"], rec["normal"], 100 * rec["ill"]))


def test_refusals_leave_every_output_untouched(dev):
    i = IDS.index("cloud N=65 K=4 B=1 ld=7/4/6 vp")
    case = CASES[i]
    blank = NR.sentinel_outputs(case["B"], case["N"], case["ldn"])
    for override in (dict(cand=None), dict(idx=None), dict(query=None), dict(B=0), dict(N=0), dict(M=0), dict(K=0), dict(N=-3),
                     dict(ldc=2), dict(ldc=17), dict(ldq=2), dict(ldq=17), dict(ldn=2), dict(B=65536)):
        rc, out, guards = _refused(dev, case, override)
        assert rc == EINVAL, override
        assert guards and same_bytes(out, blank), override
    rc, out, guards = run_raw(dev, case)                         # and the case itself is accepted
    assert rc == 0 and guards and out["err"] == 0
    # a query without a viewpoint is legal, and so is no query at all without one
    rc, _, _ = run_raw(dev, case, override=dict(viewpoint=None))
    rc2, _, _ = run_raw(dev, case, override=dict(viewpoint=None, query=None))
    assert rc == 0 and rc2 == 0


def _refused(dev, case, override):
    """The call with `override`d arguments, the buffers sized for the case itself."""
    B, N, ldn = case["B"], case["N"], case["ldn"]
    s = NR.sentinel_outputs(B, N, ldn)
    bufs = {k: cu(s[k], dev) for k in ("normal", "eig", "cov", "count")}
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    a = dict(case, **override)
    t = {k: cu(a[k], dev) for k in ("cand", "query", "idx", "dist", "n_query", "viewpoint")}
    p = _lib.ptr
    rc = _lib.load().pn2_local_pca(p(t["query"]), a["ldq"], p(t["cand"]), a["ldc"], p(t["idx"]), p(t["dist"]), a["B"], a["N"], a["M"], a["K"],
                                   a["max_d2"], p(t["n_query"]), p(t["viewpoint"]), p(bufs["normal"]), a["ldn"], p(bufs["eig"]),
                                   p(bufs["cov"]), p(bufs["count"]), p(err), _lib.stream())
    torch.cuda.synchronize()
    out = {k: bufs[k].cpu().numpy() for k in bufs}
    out["err"] = int(err.item())
    return rc, out, True


def test_wrapper_writes_into_row_columns_and_matches_the_abi(dev):
    """local_pca(out=, out_col=3): the normals land in columns 3..5 of an x, y, z, nx, ny, nz row buffer and nothing else moves; the
    [M, ld] form; eig / cov / count as returned are the C ABI's bytes."""
    i = IDS.index("cloud N=1000 K=16 B=1 ld=4/4/6 cut vp")
    case, ref = CASES[i], NR.reference(i)
    _, raw, _ = run_raw(dev, case)
    pts, idx, dist = cu(case["cand"], dev), cu(case["idx"], dev), cu(case["dist"], dev)
    rows = torch.full((1, 1000, 6), 3.5, device=dev)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    max_dist = float(np.sqrt(np.float64(case["max_d2"])))
    assert float(np.float32(max_dist ** 2)) == case["max_d2"]
    res = PN.local_pca(pts, idx, dist, max_dist=max_dist, viewpoint=cu(case["viewpoint"], dev), out=rows, out_col=3, return_eig=True,
                       return_cov=True, return_count=True, err=err)
    assert res[0] is rows and (rows[..., :3] == 3.5).all()
    assert np.array_equal(rows[..., 3:].cpu().numpy().view(np.uint32), raw["normal"][..., :3].view(np.uint32))
    assert np.array_equal(res[1].cpu().numpy().view(np.uint32), raw["eig"].view(np.uint32))
    assert np.array_equal(res[2].cpu().numpy().view(np.uint64), raw["cov"].view(np.uint64))
    assert np.array_equal(res[3].cpu().numpy(), raw["count"]) and int(err.item()) == raw["err"] == ref["err"]
    flat = PN.local_pca(pts[0], idx[0], dist[0], max_dist=max_dist, viewpoint=case["viewpoint"][0].tolist())
    assert flat.shape == (1000, 3) and np.array_equal(flat.cpu().numpy().view(np.uint32), raw["normal"][0, :, :3].view(np.uint32))
    with pytest.raises(ValueError):
        PN.local_pca(pts, idx, dist, out=rows, out_col=4)
    with pytest.raises(_lib.Pn2Error):
        PN.local_pca(pts.cpu(), idx)


def _sphere(rng, M):
    v = rng.standard_normal((M, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_estimate_normals_on_a_sphere(dev):
    """2048 points on the unit sphere, k = 16, the viewpoint at the centre: every normal points inward and lies within the angle
    the geometry allows.  The bound: a neighbour x of p at distance <= r has e . (p - x) = |p - x|^2 / (2 R) in [0, r^2 / (2 R)]
    along the radial direction e (R the sphere's radius, 1 / R its curvature), so the neighbourhood's variance along e is at
    most (r^2 / (2 R))^2 / 4 (a variable confined to an interval of length h has variance <= h^2 / 4).  Write
    e = cos(phi) u + sin(phi) w with u the eigenvector of l0 and w a unit vector in the span of the other two: then
    e^T C e >= sin^2(phi) l1, hence   sin^2(phi) <= r^4 / (16 R^2 l1),   with r the largest neighbour distance the search
    returned and l1 the row's middle eigenvalue.  (The points are float32: |p| = 1 to 2^-24, which the 1e-5 slack on sin covers.)"""
    rng = np.random.default_rng(2048)
    M, k, R = 2048, 16, 1.0
    pts = _sphere(rng, M)
    xd = cu(pts, dev)
    _, d2 = U.knn_point(k, xd[None], xd[None], return_dist=True)
    r = float(np.sqrt(d2.max().item()))
    normal, eig, count = PN.estimate_normals(xd, k=k, viewpoint=(0.0, 0.0, 0.0), return_eig=True, return_count=True)
    assert normal.shape == (M, 3) and eig.shape == (M, 3) and count.shape == (M,) and (count == k).all()
    n64, e = normal.cpu().numpy().astype(np.float64), pts.astype(np.float64)
    l = eig.cpu().numpy().astype(np.float64)
    cos = -(n64 * e).sum(1)
    assert (cos > 0).all(), "a normal points outward"
    sin2 = np.maximum(0.0, 1.0 - cos * cos)
    bound = r ** 4 / (16.0 * R * R * l[:, 1])
    assert (np.sqrt(sin2) <= np.sqrt(bound) + 1e-5).all(), float((np.sqrt(sin2) - np.sqrt(bound)).max())
    assert np.sqrt(bound).max() < 1.0, "sin(phi) <= 1 anyway: the bound says nothing for some row at this density"
    print("\nsphere: r = %.4f, largest angle %.3f deg, its bound %.3f deg" % (r, np.degrees(np.arcsin(np.sqrt(sin2))).max(),
                                                                           np.degrees(np.arcsin(np.sqrt(bound.max())))))
    sv = PN.surface_variation(eig).cpu().numpy()
    l32 = eig.cpu().numpy()
    assert np.array_equal(sv, l32[:, 0] / ((l32[:, 0] + l32[:, 1]) + l32[:, 2]))
    assert float(PN.surface_variation(torch.zeros(2, 3, device=dev)).abs().max()) == 0.0
    lin, pla, sph = PN.eigen_features(eig)
    assert np.array_equal(lin.cpu().numpy(), (l32[:, 2] - l32[:, 1]) / l32[:, 2])
    assert np.array_equal(pla.cpu().numpy(), (l32[:, 1] - l32[:, 0]) / l32[:, 2])
    assert np.array_equal(sph.cpu().numpy(), l32[:, 0] / l32[:, 2])
    assert (sv < 0.02).all() and np.abs(lin.cpu().numpy() + pla.cpu().numpy() + sph.cpu().numpy() - 1).max() <= 2.0 ** -22
    # outward with the viewpoint far outside along +z is not uniform; "origin" is the centre
    again = PN.estimate_normals(xd, k=k, viewpoint="origin")
    assert torch.equal(again.view(torch.int32), normal.view(torch.int32))


def test_graph_replay_on_new_inputs_is_byte_identical(dev):
    """estimate_normals with normals.buffers: captured once, replayed on other clouds and other device-side counts without an
    allocation; the bytes are the eager call's."""
    rng = np.random.default_rng(4)
    B, M, k = 2, 600, 9
    clouds = [rng.random((B, M, 4), np.float32) for _ in range(3)]
    counts = [np.int64([600, 311]), np.int64([17, 600]), np.int64([600, 0])]
    buf = PN.buffers(M, B=B, k=k, device=dev)
    pts = torch.zeros(B, M, 4, device=dev)
    n = torch.zeros(B, device=dev, dtype=torch.int64)

    def step():
        return PN.estimate_normals(pts, k=k, radius=0.2, viewpoint="origin", n_points=n, return_eig=True, return_cov=True,
                                   return_count=True, buffers=buf)

    def load(c, m):
        pts.copy_(cu(c, dev))
        n.copy_(cu(m, dev))

    load(clouds[0], counts[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    assert res[0] is buf.normal and res[1] is buf.eig and res[2] is buf.cov
    for c, m in zip(clouds[1:] + clouds[:1], counts[1:] + counts[:1]):
        load(c, m)
        for t in (buf.normal, buf.eig, buf.cov, buf.count):
            t.zero_()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        got = [t.clone() for t in (buf.normal, buf.eig, buf.cov, buf.count)]
        flag = int(buf.error_flag.item())
        err = torch.zeros(1, device=dev, dtype=torch.int32)
        eager = PN.estimate_normals(cu(c, dev), k=k, radius=0.2, viewpoint="origin", n_points=cu(m, dev), return_eig=True, return_cov=True,
                                    return_count=True, err=err)
        for a, b in zip(got, eager):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
        assert flag == int(err.item())
        rows = int(m[1])
        assert (got[3][1, rows:] == 0).all() and (got[0][1, rows:] == 0).all()      # rows at and beyond the count: untouched
        buf.check()
    with pytest.raises(ValueError):
        buf.error_flag.fill_(_lib.PCA_ERR_NONFINITE)
        buf.check()
