"""GPU: pn2_feature_nn2 / pn2_match_pairs against tests/match_ref.py at the C ABI, and features.match_features on top.

Everything here is held to EQUALITY: idx, the bits of dist, the pair lists and the counts.  The distance is the separately rounded
fp32 statement of the header on both sides, the selection is strict compares in index order, the compaction is prefix sums.
Outputs are prefilled with sentinels, so "not written" is checked too."""
import numpy as np
import pytest
import torch

import match_ref as R
from pointnet12_amd import _lib, features

pytestmark = pytest.mark.gpu

I64_FILL, F32_FILL = -7, -1.5
EINVAL = -1               # PN2_EINVAL of include/pn2.h
B, N, M = 2, 300, 700                                                # ragged against the 64-row query blocks and every candidate tile


def cu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


_sets = {}


def feature_set(D, kind):
    """(query [B,N,D+3], cand [B,M,D+1]) float32, read-only, made once.  "int": values 0..2 (many exact ties, all-zero rows by
    chance at small D); "real": normal deviates.  Planted in both: all-zero rows, NaN and inf rows; the columns beyond D hold junk
    that must not be read as a feature (a NaN among them)."""
    if (D, kind) not in _sets:
        rng = np.random.default_rng(100 * D + len(kind))
        q, f = np.zeros((B, N, D + 3), np.float32), np.zeros((B, M, D + 1), np.float32)
        for a in (q, f):
            a[...] = rng.integers(0, 3, a.shape) if kind == "int" else rng.normal(size=a.shape)
            a[:, :, D:] = rng.normal(size=a[:, :, D:].shape) * 50
            a[0, 3, D] = np.nan
            a[:, 5::41, :D] = 0
            a[:, 7::53, D - 1] = np.nan
            a[1, 11, 0] = np.inf
            a.setflags(write=False)
        _sets[(D, kind)] = (q, f)
    return _sets[(D, kind)]


def run_nn2(dev, q, f, D, n_query, n_cand):
    lib = _lib.load()
    qd, fd = cu(q, dev), cu(f, dev)
    nq = None if n_query is None else cu(np.int64(n_query), dev)
    nc = None if n_cand is None else cu(np.int64(n_cand), dev)
    outs = []
    for _ in range(2):
        idx = torch.full((q.shape[0], q.shape[1], 2), I64_FILL, device=dev, dtype=torch.int64)
        dist = torch.full((q.shape[0], q.shape[1], 2), F32_FILL, device=dev, dtype=torch.float32)
        rc = lib.pn2_feature_nn2(_lib.ptr(qd), q.shape[2], _lib.ptr(fd), f.shape[2], q.shape[0], q.shape[1], f.shape[1], D, _lib.ptr(nq), _lib.ptr(nc),
                                 _lib.ptr(idx), _lib.ptr(dist), _lib.stream())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((idx.cpu().numpy(), dist.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(bits(outs[0][1]), bits(outs[1][1]))          # two runs, the same bytes
    return outs[0]


COUNTS = [(None, None), ([211, 0], [700, 1]), ([300, 64], [0, 333])]      # every row; no query, a single candidate; no candidate, ragged


@pytest.mark.parametrize("D,kind", [(D, "int") for D in (1, 33, 36, 37, 64)] + [(33, "real"), (64, "real")])      # (a real-valued set per width)
def test_feature_nn2_equals_the_reference(dev, D, kind):
    q, f = feature_set(D, kind)
    for n_query, n_cand in COUNTS:
        idx, dist = run_nn2(dev, q, f, D, n_query, n_cand)
        want_idx, want_dist = R.feature_nn2(q, f, D, n_query, n_cand, np.full((B, N, 2), I64_FILL), np.full((B, N, 2), F32_FILL, np.float32))
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(bits(dist), bits(want_dist))
    if kind == "int":
        idx, _ = R.feature_nn2(q, f, D)
        assert (idx[0, 5] == M).all() and (idx[0, 7] == M).all() and (idx[:, :, 0] != 5).all()          # the planted rows took no part
        assert (idx[:, :, 0] < M).sum() > N


def test_feature_nn2_arguments(dev):
    lib = _lib.load()
    q, f = torch.zeros(1, 4, 70, device=dev), torch.zeros(1, 4, 70, device=dev)
    idx = torch.full((1, 4, 2), I64_FILL, device=dev, dtype=torch.int64)
    dist = torch.full((1, 4, 2), F32_FILL, device=dev)
    call = lambda D, ldq=70: lib.pn2_feature_nn2(_lib.ptr(q), ldq, _lib.ptr(f), 70, 1, 4, 4, D, None, None, _lib.ptr(idx), _lib.ptr(dist), _lib.stream())
    assert call(65) == _lib.PN2_EUNSUPPORTED
    assert call(0) == EINVAL and call(33, ldq=32) == EINVAL
    torch.cuda.synchronize()
    assert (idx == I64_FILL).all() and (dist == F32_FILL).all()      # nothing launched
    with pytest.raises(RuntimeError):
        features.match_features(q[0, :, :65], f[0, :, :65])


def pair_case(n_rows, rng):
    """Synthetic searches for B = 3 clouds with the device-side counts (n_rows, n_rows // 2, 0): idx int64 [3,n,2] with "none"
    entries, dist with exact ties, zeros and missing second neighbours, back with about half the rows mutual."""
    Bp, Mp = 3, 57
    idx = rng.integers(0, Mp + 1, (Bp, n_rows, 2))
    d0 = rng.integers(0, 8, (Bp, n_rows)).astype(np.float32) / 4
    d1 = d0 + rng.integers(0, 4, (Bp, n_rows)).astype(np.float32) / 4
    d1[rng.random((Bp, n_rows)) < 0.1] = np.inf
    dist = np.stack([d0, d1], 2)
    dist[idx[:, :, 0] == Mp] = np.inf
    back = rng.integers(0, n_rows + 1, (Bp, Mp, 2))
    for b in range(Bp):
        for i in rng.permutation(n_rows)[:n_rows // 2 + 1]:
            if idx[b, i, 0] < Mp:
                back[b, idx[b, i, 0], 0] = i
    return idx.astype(np.int64), dist.astype(np.float32), back.astype(np.int64), Mp, np.int64([n_rows, n_rows // 2, 0])


@pytest.mark.parametrize("n_rows", [1, 1024, 1025, 2500])
def test_match_pairs_equals_the_reference(dev, n_rows):
    """N = 1, one full compaction tile, one row more, and three tiles; mutual on and off; the ratio test off, on and at zero."""
    lib = _lib.load()
    idx, dist, back, Mp, counts = pair_case(n_rows, np.random.default_rng(n_rows))
    Bp = idx.shape[0]
    idx_d, dist_d, back_d = cu(idx, dev), cu(dist, dev), cu(back, dev)
    work = torch.full((lib.pn2_match_pairs_workspace_bytes(Bp, n_rows),), 0xA5, device=dev, dtype=torch.uint8)
    for mutual in (True, False):
        for ratio2 in (float("inf"), 0.81, 0.0):
            for n_query in (None, counts):
                runs = []
                for _ in range(2):
                    src = torch.full((Bp, n_rows), I64_FILL, device=dev, dtype=torch.int64)
                    tgt, count = src.clone(), torch.full((Bp,), I64_FILL, device=dev, dtype=torch.int64)
                    nq = None if n_query is None else cu(n_query, dev)
                    rc = lib.pn2_match_pairs(_lib.ptr(idx_d), _lib.ptr(dist_d), _lib.ptr(back_d) if mutual else None, Bp, n_rows, Mp, ratio2,
                                             _lib.ptr(nq), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(count), _lib.ptr(work), _lib.stream())
                    assert rc == 0
                    torch.cuda.synchronize()
                    runs.append((src.cpu().numpy(), tgt.cpu().numpy(), count.cpu().numpy()))
                assert all(np.array_equal(a, b) for a, b in zip(*runs))
                want = R.match_pairs(idx, dist, back if mutual else None, Mp, ratio2, n_query, fill=I64_FILL)
                for got, ref in zip(runs[0], want):
                    assert np.array_equal(got, ref)
                if n_query is not None:
                    assert runs[0][2][2] == 0                        # a cloud without rows: count 0
    s, t, c = R.match_pairs(idx, dist, back, Mp, 0.81)
    assert n_rows < 100 or 0 < c[0] < R.match_pairs(idx, dist, None, Mp, np.inf)[2][0]          # the tests do filter


def test_match_pairs_arguments(dev):
    lib = _lib.load()
    assert lib.pn2_match_pairs_workspace_bytes(0, 10) == EINVAL and lib.pn2_match_pairs_workspace_bytes(1, 0) == EINVAL
    idx = torch.zeros(1, 4, 2, device=dev, dtype=torch.int64)
    dist = torch.zeros(1, 4, 2, device=dev)
    out = torch.full((1, 4), I64_FILL, device=dev, dtype=torch.int64)
    count = torch.full((1,), I64_FILL, device=dev, dtype=torch.int64)
    work = torch.zeros(lib.pn2_match_pairs_workspace_bytes(1, 4), device=dev, dtype=torch.uint8)
    for ratio2 in (-1.0, float("nan")):
        assert lib.pn2_match_pairs(_lib.ptr(idx), _lib.ptr(dist), None, 1, 4, 4, ratio2, None, _lib.ptr(out), _lib.ptr(out), _lib.ptr(count),
                                   _lib.ptr(work), _lib.stream()) == EINVAL
    torch.cuda.synchronize()
    assert (out == I64_FILL).all() and (count == I64_FILL).all()


def test_match_features_python_layer(dev):
    """features.match_features on [B,N,D] and [N,D] inputs equals the reference's whole matcher; buffers hold the same bytes."""
    q, f = feature_set(33, "real")
    fs, ft = np.ascontiguousarray(q[:, :, :33]), np.ascontiguousarray(f[:, :, :33])
    fs[1, :200] = ft[1, 100:300] + np.float32(0.01)                 # planted true matches
    for mutual, ratio, ns, nt in ((True, 0.9, None, None), (False, None, [250, 300], [700, 650]), (True, 0.5, [0, 300], None)):
        m = features.match_features(cu(fs, dev), cu(ft, dev), mutual=mutual, ratio=ratio, n_source=ns, n_target=nt)
        want = R.match_features(fs, ft, 33, mutual, ratio, ns, nt)
        c = m.count.cpu().numpy()
        assert np.array_equal(c, want[2])
        for b in range(B):
            assert np.array_equal(m.pair_src[b, :c[b]].cpu().numpy(), want[0][b, :c[b]]) and np.array_equal(m.pair_tgt[b, :c[b]].cpu().numpy(), want[1][b, :c[b]])
            assert (m.pair_src[b, c[b]:] == -1).all()
    assert want[2][1] >= 150
    buf = features.match_buffers(N, M, B=1, device=dev)
    flat = features.match_features(cu(fs[1], dev), cu(ft[1], dev), mutual=True, ratio=0.5, buffers=buf)
    assert flat.pair_src.shape == (N,) and flat.count.shape == () and int(flat.count) == want[2][1]
    assert torch.equal(flat.pair_tgt[:int(flat.count)], m.pair_tgt[1, :c[1]])
    with pytest.raises(ValueError):
        features.match_features(cu(fs, dev), cu(ft, dev), buffers=buf)
