"""GPU: pn2_knn / pn2_knn_vote (csrc/knn.hip) and what is built on them -- knn_point, kNN grouping, propagate_labels,
FrameSegmenter.label_scan -- against the fp64 statements of tests/knn_ref.py.

On lattice inputs (tests/geometry_ref.py: every float32 operation of the distance is exact) the search must equal the fp64 answer
index for index and bit for bit, ties across the cut and coincident points included (tests/test_knn_cpu.py checks that the
cases hold plenty of both); the vote is integer arithmetic and must equal its statement on any input.

What the shapes are for (knn_kernel: 1024-candidate tiles, 256 queries per workgroup, capacities 4 / 8 / 16 / 32):
    (N, M)   (257, 33) a partly dead last wave, (300, 1023) one tile minus one, (257, 1025) plus one, (513, 2500) three tiles
    K        1, 3, 4, 5, 16, 17, 32: every capacity, each boundary between two, K = M - 1 at M = 33
    planted  the K nearest at slots {0, 1023, 1024, 1025, M - 1, ...}: across tile borders, the first and the last of all
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
import geometry_ref as R
import knn_ref as KR
from oracle import geometry as G
from pointnet12_amd import _lib, kitti
from pointnet12_amd import kitti_view as V
from pointnet12_amd import pointnet_util as U
from pointnet12_amd import synthetic as syn

pytestmark = pytest.mark.gpu

B = KR.B


def cu(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)     # (a copy: the cached reference arrays are read-only)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ search

@pytest.mark.parametrize("N,M", KR.LATTICE_CASES)
def test_knn_lattice_vs_fp64(dev, N, M):
    q, c, _ = KR.lattice_case(N, M)
    order, ds = KR.lattice_sorted(N, M)
    qd, cd = cu(q, dev), cu(c, dev)
    for K in KR.KS:
        idx, dist = U.knn_point(K, cd, qd, return_dist=True)
        assert idx.dtype == torch.int64 and idx.shape == (B, N, K) and dist.dtype == torch.float32 and dist.shape == (B, N, K)
        bad = np.argwhere(idx.cpu().numpy() != order[..., :K])
        assert len(bad) == 0, (K, len(bad), bad[:4])
        assert (dist.cpu().numpy().astype(np.float64) == ds[..., :K]).all(), K
        assert torch.equal(U.knn_point(K, cd, qd), idx)


@pytest.mark.parametrize("M", [1026, 2500])
@pytest.mark.parametrize("K", [4, 5, 16, 32])
def test_knn_planted_neighbours(dev, M, K):
    """Every candidate at least three whole units from every query, except K planted around query 0: at slots 0, 1023, 1024,
    1025, M - 1 and beyond -- across the tile borders, the first and the last of all -- at distances that come in equal pairs, in
    shuffled slot order; then as K coincident copies of the query (d = 0, indices ascending)."""
    rng = np.random.default_rng(100 * M + K)
    N = 257
    q = R.lattice(rng, 1, N)
    c = np.empty((1, M, 3), np.float32)
    c[0, :, 0] = 4 + rng.integers(0, 64, M) / 8
    c[0, :, 1:] = rng.integers(-64, 64, (M, 2)) / 8
    slots = []
    for j in [0, 1023, 1024, 1025, M - 1, 5, 64, 511, 512, 1000] + list(range(700, 740)):
        if j not in slots and j < M:
            slots.append(j)
    slots = slots[:K]
    assert len(slots) == K and {0, 1023, 1024, 1025} <= set(slots) and (M - 1 in slots or K == 4)
    for offs in ((rng.permutation(K) // 2 + 1).tolist(), [0] * K):
        cc = c.copy()
        for j, o in zip(slots, offs):
            cc[0, j] = q[0, 0] + np.float32([o / 8, 0, 0])
        idx, dist = U.knn_point(K, cu(cc, dev), cu(q, dev), return_dist=True)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        expect = sorted(zip(offs, slots))                       # ascending distance, equal distances in ascending index
        assert idx[0, 0].tolist() == [j for _, j in expect], (offs, idx[0, 0])
        assert dist[0, 0].tolist() == [(o / 8) ** 2 for o, _ in expect]
        ri, rd = KR.knn64(q, cc, K)                             # (the construction is what it claims, and the other queries)
        assert (idx == ri).all() and (dist.astype(np.float64) == rd).all()


def _continuous(kind, Bc, N):
    pts, _ = syn.kitti_batch(500 + N % 89, Bc, N) if kind == "kitti" else syn.uniform_batch(N, Bc, N)
    return np.ascontiguousarray(pts[:, :3].transpose(0, 2, 1))


def test_knn_continuous_vs_three_nn_and_oracle(dev):
    xyz = _continuous("kitti", 2, 2500)
    q, c = np.ascontiguousarray(xyz[:, :1000]), xyz
    qd, cd = cu(q, dev), cu(c, dev)
    i3, d3, _ = U.three_nn(qd, cd)
    idx, dist = U.knn_point(3, cd, qd, return_dist=True)
    assert torch.equal(idx, i3) and torch.equal(dist.view(torch.int32), d3.view(torch.int32))
    od = G.square_distance(q, c)                                # the oracle's float32 restatement of the reference's distance
    order = np.argsort(od, axis=-1, kind="stable")[..., :16]
    idx, dist = U.knn_point(16, cd, qd, return_dist=True)
    assert (idx.cpu().numpy() == order).all()
    assert (bits(dist.cpu().numpy()) == bits(np.take_along_axis(od, order, -1))).all()


def _raw_knn(dev, q, c, K, n_query=None, n_cand=None, want_dist=True):
    """pn2_knn through the C ABI into sentinel-filled buffers with a guard zone behind them -> (rc, idx, dist, guards intact)."""
    Bq, N, _ = q.shape
    M = c.shape[1]
    n = Bq * N * K
    ibuf = torch.full((n + 64,), -77, device=dev, dtype=torch.int64)
    dbuf = torch.full((n + 64,), -5.0, device=dev, dtype=torch.float32)
    qd, cd = cu(q, dev), cu(c, dev)
    nq = None if n_query is None else cu(np.int64(n_query), dev)
    nc = None if n_cand is None else cu(np.int64(n_cand), dev)
    p = _lib.ptr
    rc = _lib.load().pn2_knn(p(qd), p(cd), Bq, N, M, K, p(nq), p(nc), p(ibuf), p(dbuf) if want_dist else None, _lib.stream())
    torch.cuda.synchronize()
    intact = bool((ibuf[n:] == -77).all()) and bool((dbuf[n:] == -5.0).all()) and (want_dist or bool((dbuf == -5.0).all()))
    return rc, ibuf[:n].view(Bq, N, K).cpu().numpy(), dbuf[:n].view(Bq, N, K).cpu().numpy(), intact


def test_knn_non_finite_candidates_and_short_clouds(dev):
    rng = np.random.default_rng(11)
    N, M, K = 70, 40, 4
    q, c = R.lattice(rng, 3, N), R.lattice(rng, 3, M)
    c[:, 3] = [np.nan, 0, 0]
    c[:, 7] = [0, np.inf, 0]
    c[1, 9] = [-np.inf, 0, 0]
    rc, idx, dist, intact = _raw_knn(dev, q, c, K)
    assert rc == 0 and intact
    with np.errstate(invalid="ignore"):
        ri, rd = KR.knn64(q, c, K)                               # (fp64: inf and NaN sort behind every finite distance)
    assert np.isfinite(rd).all() and (idx == ri).all() and (dist.astype(np.float64) == rd).all()
    assert not np.isin(idx, (3, 7)).any() and not (idx[1] == 9).any()
    # fewer finite candidates than K: the unfilled slots hold (M, +inf)
    c5 = np.ascontiguousarray(c[:, :5])                          # candidate 3 is the NaN one: 4 finite
    c5[:, 1] = [np.inf, 0, 0]                                    # 3 finite
    rc, idx, dist, intact = _raw_knn(dev, q, c5, K)
    assert rc == 0 and intact and (idx[..., 3] == 5).all() and np.isposinf(dist[..., 3]).all()
    assert np.isin(idx[..., :3], (0, 2, 4)).all() and np.isfinite(dist[..., :3]).all()
    # device-side counts: n_cand = 2 < K leaves slots 2 and 3 at (M, +inf); rows at and beyond n_query keep what they held;
    # counts are clamped to [0, N] / [0, M]
    q, c = R.lattice(rng, 3, 300), R.lattice(rng, 3, 1025)
    rc, idx, dist, intact = _raw_knn(dev, q, c, K, n_query=[100, 300 + 50, -5], n_cand=[2, 1025 + 9, 1025])
    assert rc == 0 and intact
    r0i, r0d = KR.knn64(q[:1, :100], c[:1, :2], 2)
    assert (idx[0, :100, :2] == r0i[0]).all() and (dist[0, :100, :2].astype(np.float64) == r0d[0]).all()
    assert (idx[0, :100, 2:] == 1025).all() and np.isposinf(dist[0, :100, 2:]).all()
    assert (idx[0, 100:] == -77).all() and (dist[0, 100:] == -5.0).all()
    r1i, r1d = KR.knn64(q[1:2], c[1:2], K)
    assert (idx[1] == r1i[0]).all() and (dist[1].astype(np.float64) == r1d[0]).all()
    assert (idx[2] == -77).all() and (dist[2] == -5.0).all()
    # dist may be NULL
    rc, idx2, _, intact = _raw_knn(dev, q, c, K, want_dist=False)
    assert rc == 0 and intact and (idx2 == KR.knn64(q, c, K)[0]).all()


def test_knn_refusals(dev):
    q, c = cu(np.zeros((1, 8, 3), np.float32), dev), cu(np.zeros((1, 40, 3), np.float32), dev)
    out = torch.full((8 * 33,), -77, device=dev, dtype=torch.int64)
    lib, p = _lib.load(), _lib.ptr
    assert lib.pn2_knn(p(q), p(c), 1, 8, 40, 33, None, None, p(out), None, _lib.stream()) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_knn(p(q), p(c), 1, 8, 40, 41, None, None, p(out), None, _lib.stream()) in (-1, _lib.PN2_EUNSUPPORTED)
    assert lib.pn2_knn(p(q), p(c), 1, 8, 8, 9, None, None, p(out), None, _lib.stream()) == -1          # K > M
    assert lib.pn2_knn(p(q), p(c), 1, 8, 40, 0, None, None, p(out), None, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == -77).all())                              # nothing was launched
    for k in (33, 41, 0):
        with pytest.raises(RuntimeError):
            U.knn_point(k, c, q)
    with pytest.raises(RuntimeError):
        U.knn_point(9, c[:, :8], q)
    with pytest.raises(RuntimeError):
        U.propagate_labels(q, c, torch.zeros(1, 40, device=dev, dtype=torch.int64), k=33)


# -------------------------------------------------------------------------------------------------------------------- vote

def _vote_inputs(K):
    N, M = KR.VOTE_CASE
    order, ds = KR.lattice_sorted(N, M)
    return order[..., :K], ds[..., :K], KR.lattice_case(N, M)[2]


def _variant(name, N):
    """(lut, dst, out_stride, n_query) of a named variant of the vote call."""
    lut = (np.arange(KR.N_LABELS - 1, dtype=np.int32) * 3 + 100) if name != "plain" else None      # label 31 is outside it
    dst, stride, nq = None, N, None
    if name == "lut+dst+n_query":
        stride = N + 7
        dst = np.stack([np.random.default_rng(3 + b).permutation(stride)[:N] for b in range(B)]).astype(np.int32)
        dst[0, 17], dst[1, 300] = stride, -1                     # out of range on either side
        nq = [400, N + 3]
    return lut, dst, stride, nq


@functools.lru_cache(maxsize=None)
def _vote_expected(K, cut, name):
    N, M = KR.VOTE_CASE
    idx, dist, labels = _vote_inputs(K)
    lut, dst, stride, nq = _variant(name, N)
    return KR.vote_ref(idx, dist, labels, M, cut, -9, lut=lut, dst=dst, out=np.full((B, stride), -1234, np.int32), n_query=nq)


@pytest.mark.parametrize("K", KR.VOTE_KS)
def test_knn_vote_lattice_vs_statement(dev, K):
    N, M = KR.VOTE_CASE
    q, c, labels = KR.lattice_case(N, M)
    idx, dist = U.knn_point(K, cu(c, dev), cu(q, dev), return_dist=True)
    assert (idx.cpu().numpy() == _vote_inputs(K)[0]).all()
    lab_d = cu(labels, dev)
    lib, p = _lib.load(), _lib.ptr
    seen = 0
    for cut in KR.VOTE_CUTS:
        for name in ("plain", "lut", "lut+dst+n_query"):
            lut, dst, stride, nq = _variant(name, N)
            expect, expect_err = _vote_expected(K, cut, name)
            out = torch.full((B * stride + 64,), -1234, device=dev, dtype=torch.int32)
            err = torch.zeros(1, device=dev, dtype=torch.int32)
            lut_d, dst_d = (None if lut is None else cu(lut, dev)), (None if dst is None else cu(dst, dev))
            nq_d = None if nq is None else cu(np.int64(nq), dev)
            rc = lib.pn2_knn_vote(p(idx), p(dist), p(lab_d), B, N, M, K, float(np.float32(cut)), p(nq_d), -9, p(lut_d),
                                  0 if lut is None else len(lut), p(dst_d), stride, p(out), p(err), _lib.stream())
            assert rc == 0
            got = out.cpu().numpy()
            assert (got[:B * stride].reshape(B, stride) == expect).all(), (K, cut, name)
            assert (got[B * stride:] == -1234).all() and int(err.item()) == expect_err, (K, cut, name, int(err.item()), expect_err)
            seen |= expect_err
            if name == "lut+dst+n_query":
                assert expect_err & 2 and (expect == -1234).any() and (expect[0] == -1234).sum() >= N - 400
            if name == "plain":
                assert expect_err == 0
                if cut == 0.0:
                    assert 0.3 <= (expect == -9).mean() <= 0.7   # rows without a voter take the fill
    assert seen == 3                                             # both err bits were exercised


def test_propagate_labels(dev):
    """The Python entry: a DISTANCE cut-off (squared for the kernel), out / work buffers, host counts."""
    N, M = KR.VOTE_CASE
    q, c, labels = KR.lattice_case(N, M)
    idx, dist, _ = _vote_inputs(5)
    qd, cd, ld = cu(q, dev), cu(c, dev), cu(labels, dev)
    got = U.propagate_labels(qd, cd, ld, k=5, max_dist=0.25)
    assert got.dtype == torch.int32 and got.shape == (B, N)
    assert (got.cpu().numpy() == KR.vote_ref(idx, dist, labels, M, 1 / 16, -1)[0]).all()
    got = U.propagate_labels(qd, cd, ld)                         # k = 5, no cut-off
    assert (got.cpu().numpy() == KR.vote_ref(idx, dist, labels, M, np.inf, -1)[0]).all()
    out = torch.full((B, N), 55, device=dev, dtype=torch.int32)
    work = (torch.empty(B, N, 5, device=dev, dtype=torch.int64), torch.empty(B, N, 5, device=dev, dtype=torch.float32))
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    lut = cu(np.arange(KR.N_LABELS - 1, dtype=np.int32) + 1000, dev)
    res = U.propagate_labels(qd, cd, ld, k=5, max_dist=None, fill=0, lut=lut, out=out, n_query=[N, 10], n_cand=[M, 100], err=err, work=work)
    assert res is out and (work[0][0].cpu().numpy() == idx[0]).all()
    i1, d1 = KR.knn64(q[1:, :10], c[1:, :100], 5)
    expect, e = KR.vote_ref(np.concatenate([idx[:1, :10], i1]), np.concatenate([dist[:1, :10], d1]), labels, M, np.inf, 0,
                            lut=np.arange(KR.N_LABELS - 1, dtype=np.int32) + 1000)
    assert (out[1, :10].cpu().numpy() == expect[1]).all() and (out[1, 10:] == 55).all()
    assert (out[0].cpu().numpy() == KR.vote_ref(idx[:1], dist[:1], labels[:1], M, np.inf, 0,
                                               lut=np.arange(KR.N_LABELS - 1, dtype=np.int32) + 1000)[0][0]).all()


# ---------------------------------------------------------------------------------------------------------------- modules

def test_set_abstraction_with_knn_equals_ball_module_on_knn_indices(dev, monkeypatch):
    """PointNetSetAbstraction(knn=True) against the same module built knn=False, sharing its weights, whose ball query is
    replaced by the fp64 statement's indices: bit-equal forward, gradients within the backward's run-to-run noise."""
    Bm, N, S, K, D = 2, 512, 128, 16, 3
    rng = np.random.default_rng(5)
    xyz = cu(R.lattice(rng, Bm, N).transpose(0, 2, 1), dev)      # [B, 3, N]; lattice: the fp64 neighbours ARE the kernel's
    feats = torch.randn(Bm, D, N, generator=torch.Generator().manual_seed(1))
    start = torch.tensor([3, 77])
    torch.manual_seed(0)
    knn_mod = U.PointNetSetAbstraction(S, 0.2, K, 3 + D, [32, 64], False, knn=True).to(dev).train()
    ball_mod = U.PointNetSetAbstraction(S, 0.2, K, 3 + D, [32, 64], False).to(dev).train()
    ball_mod.load_state_dict(knn_mod.state_dict())
    calls = []

    def knn64_for_ball(radius, nsample, pts, new_pts):
        calls.append(nsample)
        return cu(KR.knn64(new_pts.cpu().numpy(), pts.cpu().numpy(), nsample)[0], dev)
    gw = torch.randn(Bm, 64, S, generator=torch.Generator().manual_seed(2)).to(dev)
    res = []
    for mod in (knn_mod, ball_mod):
        f = feats.clone().to(dev).requires_grad_(True)
        with monkeypatch.context() as mp:
            if mod is ball_mod:
                mp.setattr(U, "query_ball_point", knn64_for_ball)
            new_xyz, out = mod(xyz, f, fps_start=start)
        (out * gw).sum().backward()
        res.append((new_xyz.detach().clone(), out.detach().clone(), f.grad.clone(), [p.grad.clone() for p in mod.parameters()]))
    assert calls == [K]
    (xa, oa, fa, pa), (xb, ob, fb, pb) = res
    assert torch.equal(xa, xb) and torch.equal(oa, ob) and float(oa.abs().max()) > 0
    names = ["input"] + [n for n, _ in knn_mod.named_parameters()]
    for n, a, b in zip(names, [fa] + pa, [fb] + pb):
        scale = float(a.abs().max())
        if scale < 1e-7:                                         # (zero in exact arithmetic: conv biases before a BatchNorm)
            continue
        print("%s: gradient difference %.3g of scale %.3g" % (n, float((a - b).abs().max()), scale))
        assert float((a - b).abs().max()) <= 1e-5 * scale, n
    # sample_and_group(knn=True): the groups are knn_point's
    xyz_cl = xyz.permute(0, 2, 1).contiguous()
    torch.manual_seed(4)
    new_xyz, new_points, grouped_xyz, fps_idx = U.sample_and_group(S, 0.2, K, xyz_cl, None, returnfps=True, knn=True)
    idx = U.knn_point(K, xyz_cl, new_xyz)
    assert torch.equal(grouped_xyz, U.index_points(xyz_cl, idx)) and new_points.shape == (Bm, S, K, 3)
    assert torch.equal(new_points, grouped_xyz - new_xyz[:, :, None, :])


class _KnnNet(torch.nn.Module):
    """Two kNN set-abstraction levels: [B, 6, N] -> [B, 128, 32]."""

    def __init__(self):
        super().__init__()
        self.sa1 = U.PointNetSetAbstraction(128, 0.2, 16, 3 + 3, [32, 64], False, knn=True)
        self.sa2 = U.PointNetSetAbstraction(32, 0.4, 8, 64 + 3, [64, 128], False, knn=True)

    def features(self, pts):
        l1_xyz, l1 = self.sa1(pts[:, :3, :], pts[:, 3:, :])
        return self.sa2(l1_xyz, l1)[1]

    def forward(self, pts):
        return F.log_softmax(self.features(pts).mean(2), 1)


def _knn_net_losses(dev, mode):
    from pointnet12_amd import parallel
    from pointnet12_amd.graph import GraphedStep
    gen = torch.Generator().manual_seed(9)
    pts = (torch.rand(2, 6, 512, generator=gen) * 2 - 1).to(dev)
    labels = torch.tensor([5, 100]).to(dev)
    torch.manual_seed(0)
    net = _KnnNet().to(dev).train()
    bucket = parallel.FlatGradBucket(net)

    def compute():
        bucket.zero()
        loss = F.nll_loss(net(pts), labels)
        loss.backward()
        return loss
    torch.manual_seed(31)
    if mode == "eager":
        for _ in range(2):                                       # the captured variants run 2 eager warm-up steps: same BN history
            compute()
        step = compute
    elif mode == "captured":
        step = GraphedStep(compute, dev, warmup=2)
    else:
        step = GraphedStep(compute, dev, warmup=2, geometry_fn=lambda: net.features(pts))
    losses = [float(step().detach()) for _ in range(3)]
    return losses, bucket.flat.clone()


def test_knn_network_through_the_captured_step(dev):
    """A two-level network of kNN modules: the captured step (graph.py) gives the eager loss, and so does the captured step
    with the next batch's geometry recorded on the side stream (knn_point goes through the geometry tape)."""
    (le, ge), (lc, gc), (lp, gp) = (_knn_net_losses(dev, m) for m in ("eager", "captured", "prefetch"))
    print("losses eager %s captured %s prefetch %s" % (le, lc, lp))
    assert all(np.isfinite(le)) and float(ge.abs().max()) > 0
    for other in (lc, lp):
        assert max(abs(a - b) for a, b in zip(le, other)) <= 1e-5


# ------------------------------------------------------------------------------------------------------------- label_scan

class _SignStub(torch.nn.Module):
    """A stand-in for the network: [1, 4, n] -> log-probabilities [1, n, 4] that depend on the sign of x alone (class 2 where
    x > 0, class 1 elsewhere)."""

    def forward(self, x):
        pos = (x[:, 0, :] > 0).unsqueeze(-1)
        logits = torch.where(pos, x.new_tensor([0.0, 0.0, 9.0, 0.0]), x.new_tensor([0.0, 9.0, 0.0, 0.0]))
        return torch.log_softmax(logits, -1)


def test_label_scan(dev, monkeypatch, tmp_path):
    g = golden("g18_kitti_view.npz")
    rng = np.random.default_rng(21)
    M, n = 3000, 1024
    # whole eighths up to +-16: float32 distances are exact, so the fp64 statement's neighbours are the kernel's.  Nothing lies
    # within 2 m of the plane x = 0: every voter within max_dist = 1 m of a row is on the row's own side
    raw = np.empty((M, 4), np.float32)
    raw[:, 0] = rng.choice([-1, 1], M) * rng.integers(16, 96, M) / 8
    raw[:, 1] = rng.integers(-24, 25, M) / 8
    raw[:, 2] = rng.integers(-8, 9, M) / 8
    raw[:, 3] = rng.integers(0, 100, M) / 100
    words = rng.choice(np.uint32([0, 1, 2, 5]), M, p=[0.1, 0.3, 0.3, 0.3]) | np.uint32(7 << 16)     # (an instance id above)
    sf = kitti.ScanFilter({0: 0, 1: 1, 2: 2, 5: 3}, "all", x_range=(-11, 11), device=dev)
    lut_np = np.int32([40, 44, 48, 70])
    lut = cu(lut_np, dev)
    seg = V.FrameSegmenter(_SignStub().to(dev), V.Calibration(g["R"], g["T"], g["P"]), g["colors"], npoints=n)
    raw_d, words_d = cu(raw, dev), cu(words.view(np.int32), dev)
    out = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=torch.Generator(device=dev).manual_seed(3), k=5, max_dist=1.0, lut=lut)
    torch.cuda.synchronize()
    assert int(seg.error_flag.item()) == 0 and int(sf.error_flag.item()) == 0
    scan_labels = out["scan_labels"].cpu().numpy().copy()
    assert scan_labels.dtype == np.int32 and scan_labels.shape == (M,)
    count = int(out["count"].item())
    keep = ((words & 0xFFFF) != 0) & (raw[:, 0] > -11) & (raw[:, 0] < 11)
    index = out["index"][:count].cpu().numpy()
    assert count == keep.sum() and (index == np.flatnonzero(keep)).all() and 0.5 * M < count < 0.95 * M
    cand, pred = out["pts_3d"].cpu().numpy(), out["pred"].cpu().numpy()
    assert ((pred == 2) == (cand[:, 0] > 0)).all() and ((pred == 1) == (cand[:, 0] < 0)).all()
    drawn = len({r.tobytes() for r in cand})
    assert drawn < 0.9 * n                                       # duplicates among the candidates: the draw is with replacement
    kept_xyz = raw[index, :3]
    # every dropped row is 0
    assert (scan_labels[~keep] == 0).all()
    # every kept row whose nearest candidate lies on its own side (within reach) carries lut[class of its sign]
    ni, nd = KR.knn64(kept_xyz[None], cand[None], 1)
    own = np.sign(cand[ni[0, :, 0], 0]) == np.sign(kept_xyz[:, 0])
    reach = nd[0, :, 0] <= 1.0
    assert own.all() and reach.mean() > 0.99
    want = np.where(kept_xyz[:, 0] > 0, lut_np[2], lut_np[1])
    assert (scan_labels[index][reach] == want[reach]).all() and (scan_labels[index][~reach] == 0).all()
    undrawn = nd[0, :, 0] > 0
    assert 0.2 < undrawn.mean() < 0.9                            # rows the network never saw, labelled all the same
    # the whole tensor is the statement's, on the tensors the frame returned
    i5, d5 = KR.knn64(kept_xyz[None], cand[None], 5)
    expect, e = KR.vote_ref(i5, d5, pred[None], n, 1.0, 0, lut=lut_np, dst=index[None], out=np.zeros((1, M), np.int32))
    assert e == 0 and (scan_labels == expect[0]).all()
    # an equally seeded generator: identical bytes, and nothing is read back on the way

    def forbidden(*args, **kwargs):
        raise AssertionError("label_scan read something back")
    with monkeypatch.context() as mp:
        for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "nonzero"):
            mp.setattr(torch.Tensor, name, forbidden)
        mp.setattr(torch.cuda, "synchronize", forbidden)
        again = seg.label_scan(raw_d, words_d, scan_filter=sf, rng=torch.Generator(device=dev).manual_seed(3), k=5, max_dist=1.0, lut=lut)
    torch.cuda.synchronize()
    assert again["scan_labels"].cpu().numpy().tobytes() == scan_labels.tobytes()
    fn = str(tmp_path / "000000.label")                          # and the file
    kitti.write_labels(fn, again["scan_labels"])
    assert ((np.fromfile(fn, np.uint32) & 0xFFFF) == scan_labels).all()
