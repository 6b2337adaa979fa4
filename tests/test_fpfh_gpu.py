"""GPU: pn2_spfh / pn2_fpfh (csrc/fpfh.hip) and pointnet12_amd/features.py against the numpy statement of the rule
(tests/fpfh_ref.py; include/pn2.h, "FPFH").  THE BOUNDS, stated before any run:

  BINS.    The SPFH bytes EQUAL the reference's on every row the reference does not flag.  A row is flagged when one of its pairs
           has a t1, t2 or t3 within 2^-30 of an integer edge 1..10 (for t1 also the wrap ends 0 and 11, unless atan2's first
           argument is exactly 0): everything but atan2 is correctly rounded fp64 on both sides, and an atan2 that differs from
           libm's by a few ulp moves t1 by about 1e-15.  Flagged rows are at most 1 % of the rows of each case (asserted).
  FINISH.  pn2_fpfh on the DEVICE'S OWN SPFH bytes against fpfh_ref.finish on those bytes: within 1 ulp of float32.  Every term
           is non-negative and there are at most 32 of them with three roundings each, so the fp64 relative error of either side is
           below 2^-46 and the two float32 roundings can differ only across a midpoint.  Expected: equal in every bit (the same
           operations in the same order, correctly rounded divide); the count of unequal elements is printed.
  THIRDS.  Every third of a row with a voter and m > 0 sums to 200 within 1e-4 (eleven float32 roundings of values that add up
           to 200: at most 11 * 2^-25 * 200 = 6.6e-5, added in fp64).
"""
import math

import numpy as np
import pytest
import torch

import fpfh_ref as F
import icp_ref
from pointnet12_amd import _lib
from pointnet12_amd import features as FT
from pointnet12_amd import neighbors as NB
from pointnet12_amd import pointnet_util as U

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
SPFH_FILL, FPFH_FILL = 0xAB, 7.0
unequal_total = [0, 0]                                           # (unequal float32 elements, elements compared) over the sweep


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)     # (a copy: the cached arrays are read-only)


def run_raw(dev, pts, nrm, normal_col, idx, max_d2=np.inf, n_points=None, override=None):
    """Both kernels through the C ABI on sentinel-filled outputs -> (rc_spfh, rc_fpfh, spfh bytes, fpfh, err_spfh, err_fpfh).
    ``nrm`` None: the normals are columns normal_col.. of ``pts``."""
    a = dict(B=pts.shape[0], M=pts.shape[1], K=idx.shape[2], ldp=pts.shape[2], ldn=(pts if nrm is None else nrm).shape[2],
             normal_col=normal_col, max_d2=float(max_d2), points=True, normals=True, idx=True, out=True, spfh=True)
    a.update(override or {})
    B, M = pts.shape[:2]
    p = _lib.ptr
    tp = cu(pts, dev)
    tn = tp if nrm is None else cu(nrm, dev)
    ti, tc = cu(idx, dev), cu(None if n_points is None else np.asarray(n_points, np.int64), dev)
    spfh = torch.full((B, M, 36), SPFH_FILL, device=dev, dtype=torch.uint8)
    fpfh = torch.full((B, M, 33), FPFH_FILL, device=dev, dtype=torch.float32)
    e1, e2 = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
    g = lambda t, k: p(t) if a[k] else None
    lib = _lib.load()
    rc1 = lib.pn2_spfh(g(tp, "points"), a["ldp"], g(tn, "normals"), a["ldn"], a["normal_col"], g(ti, "idx"), a["B"], a["M"], a["K"],
                       a["max_d2"], p(tc), g(spfh, "out"), p(e1), _lib.stream())
    rc2 = lib.pn2_fpfh(g(tp, "points"), a["ldp"], g(ti, "idx"), g(spfh, "spfh"), a["B"], a["M"], a["K"], a["max_d2"], p(tc),
                       g(fpfh, "out"), p(e2), _lib.stream())
    torch.cuda.synchronize()
    return rc1, rc2, spfh.cpu().numpy(), fpfh.cpu().numpy(), int(e1.item()), int(e2.item())


def check_against_rule(dev, pts, nrm, normal_col, idx, max_d2=np.inf, n_points=None, what=""):
    """Runs both kernels and holds them to the three bounds of this file's docstring; returns the device's outputs."""
    B, M = pts.shape[:2]
    rc1, rc2, spfh, fpfh, e1, e2 = run_raw(dev, pts, nrm, normal_col, idx, max_d2, n_points)
    assert rc1 == 0 and rc2 == 0, what
    nr = (pts if nrm is None else nrm)[:, :, normal_col:normal_col + 3]
    ref, flagged, err = F.spfh(pts, nr, idx, max_d2, n_points, before=np.full((B, M, 36), SPFH_FILL, np.uint8))
    assert flagged.sum() <= 0.01 * B * M, (what, int(flagged.sum()))
    assert np.array_equal(spfh[~flagged], ref[~flagged]), (what, np.argwhere((spfh != ref).any(-1) & ~flagged)[:5])
    if not flagged.any():
        assert e1 == err, what
    fin, voters, err2 = F.finish(pts, idx, spfh, max_d2, n_points, before=np.full((B, M, 33), FPFH_FILL, np.float32))
    assert e2 == err2, what
    assert not np.isnan(fpfh).any() and (fpfh >= 0).all(), what
    ulps = np.abs(fpfh.view(np.int32).astype(np.int64) - fin.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, (what, int(ulps.max()))
    unequal_total[0] += int((ulps != 0).sum())
    unequal_total[1] += ulps.size
    ns = [M] * B if n_points is None else [max(0, min(M, int(v))) for v in n_points]
    for b in range(B):
        live = (voters[b, :ns[b]] > 0) & (spfh[b, :ns[b], 33] > 0)
        thirds = fpfh[b, :ns[b]][live].astype(np.float64).reshape(-1, 3, 11).sum(-1)
        assert thirds.size == 0 or np.abs(thirds - 200.0).max() <= 1e-4, what
    return spfh, fpfh, e1, e2


def _cloud(N, seed):
    pts, nrm = F.wavy_sheet(N, seed)
    return pts, nrm


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_both_kernels_vs_rule_over_shapes(dev, N):
    """N x K in {1, 2, 8, 16, 17, 32} x ldp in {3, 4, 6}, three clouds with the device-side counts (N, 2, 0) whose lists still name
    rows beyond the count; the normals as a buffer of their own and as columns 3..5 of the points; B = 1 without counts."""
    clouds = [_cloud(N, 5 + b) for b in range(3)]
    rng = np.random.default_rng(N)
    for K in (1, 2, 8, 16, 17, 32):
        idx = np.stack([F.knn_self(c[0], K) for c in clouds])
        for ldp in (3, 4, 6):
            pts = rng.random((3, N, ldp)).astype(np.float32)
            pts[:, :, :3] = np.stack([c[0] for c in clouds])
            nrm = np.stack([c[1] for c in clouds])
            what = "N=%d K=%d ldp=%d" % (N, K, ldp)
            if ldp == 6:
                pts[:, :, 3:] = nrm
                a = check_against_rule(dev, pts, None, 3, idx, np.inf, (N, 2, 0), what + " rows")
                wide = np.concatenate([rng.random((3, N, 2)).astype(np.float32), nrm], 2)           # ldn = 5, normal_col = 2
                b = check_against_rule(dev, pts, wide, 2, idx, np.inf, (N, 2, 0), what + " own")
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
            else:
                spfh, fpfh, _, _ = check_against_rule(dev, pts, nrm, 0, idx, 0.09 if K == 16 else np.inf, (N, 2, 0), what)
                assert (spfh[1, 2:] == SPFH_FILL).all() and (spfh[2] == SPFH_FILL).all()            # rows at and beyond the count
                assert (fpfh[1, 2:] == FPFH_FILL).all() and (fpfh[2] == FPFH_FILL).all()
        if K == 16:
            check_against_rule(dev, pts[:1], nrm[:1], 0, idx[:1], np.inf, None, "N=%d K=16 B=1" % N)


def test_sheet_and_lattice_flag_nothing_and_match(dev):
    """The two inputs of the BINS bound: the 1 024-point wavy sheet at K = 16 and the 5 x 5 x 3 lattice with normals from eight fixed
    directions (exact ties of |a1| and |a2|, zero |v|, antiparallel normals) at K = 32."""
    for (pts, nrm), K in ((F.wavy_sheet(), 16), (F.lattice(), 32)):
        idx = F.knn_self(pts, K)
        _, flagged, _ = F.spfh_cloud(pts, nrm, idx)
        assert not flagged.any()
        check_against_rule(dev, pts[None], nrm[None], 0, idx[None], np.inf, None, "K=%d" % K)
    print("\nfinish: %d of %d float32 elements differ from the reference so far" % tuple(unequal_total))


def test_lists_from_the_package_searches(dev):
    """Lists as knn_point and GridIndex.query_self (both visit orders) write them, through the Python layer."""
    pts, nrm = F.wavy_sheet()
    xd, nd = cu(pts, dev), cu(nrm, dev)
    lists = {"knn": (U.knn_point(16, xd[None], xd[None])[0], None)}
    for order in (True, False):
        index = NB.GridIndex(radius=0.3).build(xd)
        lists["grid sorted=%s" % order] = (index.query_self(16, visit_sorted=order), 0.3)
    assert torch.equal(lists["grid sorted=True"][0], lists["grid sorted=False"][0])
    for name, (idx, radius) in lists.items():
        assert idx.shape == (1024, 16) and idx.dtype == torch.int64
        err = torch.zeros(1, device=dev, dtype=torch.int32)
        out, spfh = FT.fpfh(xd, nd, idx, max_dist=radius, return_spfh=True, err=err)
        assert out.shape == (1024, 33) and spfh.shape == (1024, 36) and spfh.dtype == torch.uint8
        max_d2 = np.inf if radius is None else np.float32(radius ** 2)
        raw = check_against_rule(dev, pts[None], nrm[None], 0, idx.cpu().numpy()[None], max_d2, None, name)
        assert np.array_equal(spfh.cpu().numpy(), raw[0][0]) and np.array_equal(out.cpu().numpy().view(np.int32), raw[1][0].view(np.int32))
        assert int(err.item()) == raw[2] | raw[3]
        assert torch.equal(FT.spfh(xd, nd, idx, max_dist=radius), spfh)
        c, m = FT.spfh_counts(spfh)
        assert c.dtype == torch.int32 and c.shape == (1024, 33) and (c[:, :11].sum(1) == m).all() and (c[:, 22:].sum(1) == m).all()
    rows = torch.cat([xd, nd], 1)                                   # x y z nx ny nz, read where it lies
    assert torch.equal(FT.fpfh(rows, rows, lists["knn"][0], normal_col=3), FT.fpfh(xd, nd, lists["knn"][0]))


def test_hand_made_lists_and_planted_rows(dev):
    """Padding (idx = M), negative indices, repeats, the row itself, exact duplicate points, indices at and beyond n_points, rows
    beyond max_d2; NaN / inf points and NaN normals (pair skipped, ERR_NONFINITE), zero normals (pair skipped); a row with no pair
    (zeros, ERR_EMPTY)."""
    lp, ln = F.lattice()
    pts, nrm = np.array(lp), np.array(ln)
    M, K = len(pts), 8
    rng = np.random.default_rng(12)
    idx = rng.integers(-1, M + 2, (M, K))
    idx[:, 0] = np.arange(M)
    idx[:, 3] = idx[:, 2]                                            # a candidate listed twice
    pts[11] = pts[10]
    idx[10, 1], idx[11, 1] = 11, 10                                  # exact duplicates
    idx[20, :] = M                                                   # nothing but padding
    idx[21, :] = 21                                                  # nothing but itself
    idx[7, 4], idx[8, 4] = 8, 6                                      # rows 7 and 8 (planted normals below) each have a neighbour in reach
    clean = check_against_rule(dev, pts[None], nrm[None], 0, idx[None], 0.3, (70,), "hand-made")
    c, m = F.counts(clean[0][0])
    assert m[20] == 0 and m[21] == 0 and (clean[0][0, 20] == 0).all() and (clean[1][0, 21] == 0).all()
    assert clean[2] == F.ERR_EMPTY and clean[3] == F.ERR_EMPTY and 0 < m[:70].max() <= K
    assert (clean[0][0, 70:] == SPFH_FILL).all() and (clean[1][0, 70:] == FPFH_FILL).all()
    pts[5, 0], pts[6, 2] = np.nan, np.inf
    planted = check_against_rule(dev, pts[None], nrm[None], 0, idx[None], 0.3, (70,), "planted points")
    assert planted[2] & F.ERR_NONFINITE and planted[3] & F.ERR_NONFINITE and F.counts(planted[0][0])[1][5] == 0
    pts[5], pts[6] = lp[5], lp[6]
    nrm[7, 1], nrm[8] = np.nan, 0.0
    bad = check_against_rule(dev, pts[None], nrm[None], 0, idx[None], 0.3, (70,), "planted normals")
    assert bad[2] & F.ERR_NONFINITE and not bad[3] & F.ERR_NONFINITE                    # (pn2_fpfh reads no normals)
    assert F.counts(bad[0][0])[1][8] == 0 and F.counts(bad[0][0])[1][7] == 0
    nrm[7] = ln[7]
    zero = check_against_rule(dev, pts[None], nrm[None], 0, idx[None], 0.3, (70,), "a zero normal")
    assert zero[2] == F.ERR_EMPTY                                                       # lost without a flag of its own


def test_antiparallel_normals_fall_into_bin_10(dev):
    pts = cu(np.float32([[0, 0, 0], [1, 0, 0]]), dev)
    nrm = cu(np.float32([[0, 0, 1], [0, 0, -1]]), dev)
    idx = cu(np.int64([[1], [0]]), dev)
    c, m = FT.spfh_counts(FT.spfh(pts, nrm, idx))
    assert m.tolist() == [1, 1] and c[:, 10].tolist() == [1, 1] and c[:, :10].sum().item() == 0
    assert c[:, 16].tolist() == [1, 1] and c[:, 27].tolist() == [1, 1]
    f = FT.fpfh(pts, nrm, idx)
    assert f[:, [10, 16, 27]].eq(200.0).all() and f.sum().item() == 1200.0


def test_refusals_leave_the_outputs_untouched(dev):
    pts, nrm = F.wavy_sheet(65)
    rows = np.concatenate([pts, nrm], 1)[None]
    idx = F.knn_self(pts, 4)[None]
    cases = [(dict(points=False), EINVAL), (dict(idx=False), EINVAL), (dict(out=False), EINVAL),
             (dict(K=0), EINVAL), (dict(K=-1), EINVAL), (dict(K=33), EUNSUPPORTED), (dict(ldp=2), EINVAL), (dict(ldp=17), EINVAL),
             (dict(max_d2=-1.0), EINVAL), (dict(max_d2=math.nan), EINVAL), (dict(B=0), EINVAL), (dict(M=0), EINVAL), (dict(B=65536), EINVAL)]
    for override, want in cases:
        rc1, rc2, spfh, fpfh, e1, e2 = run_raw(dev, rows, None, 3, idx, override=override)
        assert rc1 == want and rc2 == want, override
        assert (spfh == SPFH_FILL).all() and (fpfh == FPFH_FILL).all() and e1 == 0 and e2 == 0, override
    for override in (dict(normals=False), dict(ldn=2), dict(ldn=17), dict(normal_col=4), dict(normal_col=-1)):      # pn2_spfh's own
        rc1, _, spfh, _, e1, _ = run_raw(dev, rows, None, 3, idx, override=override)
        assert rc1 == EINVAL and (spfh == SPFH_FILL).all() and e1 == 0, override
    _, rc2, _, fpfh, _, e2 = run_raw(dev, rows, None, 3, idx, override=dict(spfh=False))                   # pn2_fpfh's own
    assert rc2 == EINVAL and (fpfh == FPFH_FILL).all() and e2 == 0
    rc1, rc2, _, _, e1, e2 = run_raw(dev, rows, None, 3, idx, max_d2=0.0)                                  # a zero cut-off is legal: no pair
    assert rc1 == 0 and rc2 == 0 and e1 == F.ERR_EMPTY and e2 == F.ERR_EMPTY
    xd, nd, ix = cu(pts, dev), cu(nrm, dev), cu(idx[0], dev)
    for args in ((xd.cpu(), nd, ix), (xd, nd.cpu(), ix), (xd, nd, ix.cpu())):
        with pytest.raises(_lib.Pn2Error):
            FT.fpfh(*args)
        with pytest.raises(_lib.Pn2Error):
            FT.spfh(*args)
    with pytest.raises(_lib.Pn2Error):
        FT.compute_fpfh(xd.cpu(), 0.5)
    with pytest.raises(ValueError):
        FT.fpfh(xd, nd, ix, normal_col=1)
    with pytest.raises(RuntimeError):
        FT.fpfh(xd, nd, torch.zeros(65, 33, device=dev, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        FT.compute_fpfh(xd, 0.5, k=33)
    # rows at and beyond n_points keep what they held, through the Python layer: zeros when it allocates
    part = FT.fpfh(xd, nd, ix, n_points=[40])
    assert (part[40:] == 0).all() and part[:40].sum().item() > 0


def _capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    return graph, res


@pytest.mark.parametrize("search", ["grid", "brute"])
def test_two_runs_are_identical_and_a_graph_replays_on_new_inputs(dev, search):
    """compute_fpfh with features.buffers: captured once (one graph, serial launches), replayed on other clouds and other
    device-side counts without an allocation; the bytes are the eager call's, and two eager runs are byte-identical."""
    rng = np.random.default_rng(8)
    B, M, k = 2, 600, 12
    clouds = [np.concatenate([rng.random((B, M, 2)) * 2.0, 0.1 * rng.random((B, M, 1)), rng.random((B, M, 1))], 2).astype(np.float32)
              for _ in range(3)]
    counts = [np.int64([600, 311]), np.int64([17, 600]), np.int64([600, 0])]
    buf = FT.buffers(M, B=B, k=k, device=dev, search=search)
    pts = torch.zeros(B, M, 4, device=dev)
    n = torch.zeros(B, device=dev, dtype=torch.int64)
    view = torch.tensor([[1.0, 1.0, 5.0]] * B, device=dev)

    def step():
        return FT.compute_fpfh(pts, 0.3, k=k, normal_k=10, viewpoint=view, n_points=n, search=search, buffers=buf)

    def load(c, m):
        pts.copy_(cu(c, dev))
        n.copy_(cu(m, dev))

    load(clouds[0], counts[0])
    graph, res = _capture(step)
    assert res is buf.fpfh
    for c, m in zip(clouds[1:] + clouds[:1], counts[1:] + counts[:1]):
        load(c, m)
        buf.fpfh.zero_()
        buf.spfh.zero_()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        replayed, replayed_spfh = buf.fpfh.clone(), buf.spfh.clone()
        buf.check()
        eager = FT.compute_fpfh(pts, 0.3, k=k, normal_k=10, viewpoint=view, n_points=n, search=search)
        again = FT.compute_fpfh(pts, 0.3, k=k, normal_k=10, viewpoint=view, n_points=n, search=search)
        assert eager.shape == (B, M, 33) and torch.equal(eager.view(torch.int32), again.view(torch.int32))
        assert torch.equal(eager.view(torch.int32), replayed.view(torch.int32))
        assert replayed[0, :int(m[0])].sum().item() > 0 and (replayed_spfh[1, int(m[1]):] == 0).all()
    with pytest.raises(ValueError):
        FT.compute_fpfh(pts, 0.3, k=k, buffers=FT.buffers(M, B=B, k=k, device=dev, search="brute" if search == "grid" else "grid"),
                        search=search)


def test_descriptors_survive_a_rigid_motion(dev):
    """End to end, small: the 2 048-row wavy-sheet cloud of the ICP tests and the SAME rows after 3 degrees about (1, 2, 3) plus a
    translation, compute_fpfh with estimated normals (oriented towards a viewpoint that moves with the cloud).  The descriptors of
    matching rows differ only through the normals' and the bins' rounding: their median L1 distance lies below the median L1
    distance between a row and a random other row.  Two numbers measured in the same test, no constant."""
    _, tgt, _ = icp_ref.sheets_pair()
    a = tgt[0].astype(np.float64)
    moved = (a @ icp_ref.PLANTED_R.T + icp_ref.PLANTED_T).astype(np.float32)
    eye = np.array([0.0, 0.0, 8.0])
    radius = 0.5
    fa = FT.compute_fpfh(cu(tgt[0], dev), radius, k=32, viewpoint=eye.tolist())
    fb = FT.compute_fpfh(cu(moved, dev), radius, k=32, viewpoint=(icp_ref.PLANTED_R @ eye + icp_ref.PLANTED_T).tolist())
    assert fa.shape == (2048, 33) and fb.shape == (2048, 33)
    other = torch.from_numpy(np.random.default_rng(3).permutation(2048)).to(dev)
    same = (fa - fb).abs().sum(1).median().item()
    rand = (fa - fb[other]).abs().sum(1).median().item()
    print("\nrigid motion: median L1 between matching rows %.6g, between a row and a random other row %.6g" % (same, rand))
    assert same < rand
