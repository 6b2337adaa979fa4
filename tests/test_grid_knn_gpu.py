"""GPU: pn2_grid_build + pn2_grid_knn write exactly what tests/grid_knn_ref.py states -- idx, the bits of dist and count EQUAL the
reference; there is no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest
import torch

import grid_knn_ref as R
from geometry_ref import lattice
from pointnet12_amd import _lib, neighbors
from pointnet12_amd import normals as PN
from pointnet12_amd import pointnet_util as U

pytestmark = pytest.mark.gpu

IDX_FILL, DIST_FILL, COUNT_FILL = -77, -3.5, -9          # what the outputs hold before a call: rows a call must not touch keep it


def cu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)               # (a contiguous, writable copy: the shared cases are read-only)


def triple(v):
    return (ctypes.c_double * 3)(*np.broadcast_to(np.asarray(v, np.float64), (3,)))


def grid_search(dev, cand, query, K, max_d2, origin=0.0, cell=None, n_query=None, n_cand=None, flags=0, want=("dist", "count", "err"),
                fill=0xA5):
    """pn2_grid_build then pn2_grid_knn at the C ABI on numpy inputs -> dict of numpy outputs (idx, dist, count as the device
    left them, prefilled with the patterns above) and the two err words."""
    lib = _lib.load()
    cand = np.asarray(cand, np.float32)
    B, M, ldc = cand.shape
    N = M if query is None else query.shape[1]
    cell = R.default_cell(max_d2) if cell is None else cell
    o, c = triple(origin), triple(cell)
    dc = cu(cand, dev)
    dq = None if query is None else cu(np.asarray(query, np.float32), dev)
    nq = None if n_query is None else cu(np.asarray(n_query, np.int64), dev)
    nc = None if n_cand is None else cu(np.asarray(n_cand, np.int64), dev)
    ws = torch.full((lib.pn2_grid_workspace_bytes(B, M),), fill, device=dev, dtype=torch.uint8)          # (it may hold anything)
    idx = torch.full((B, N, K), IDX_FILL, device=dev, dtype=torch.int64)
    dist = torch.full((B, N, K), DIST_FILL, device=dev, dtype=torch.float32) if "dist" in want else None
    count = torch.full((B, N), COUNT_FILL, device=dev, dtype=torch.int32) if "count" in want else None
    eb = torch.zeros(1, device=dev, dtype=torch.int32) if "err" in want else None
    eq = torch.zeros(1, device=dev, dtype=torch.int32) if "err" in want else None
    p, st = _lib.ptr, _lib.stream()
    _lib.check(lib.pn2_grid_build(p(dc), ldc, B, M, p(nc), ctypes.addressof(o), ctypes.addressof(c), p(eb), p(ws), st), "pn2_grid_build")
    _lib.check(lib.pn2_grid_knn(p(dq), 0 if query is None else query.shape[2], B, N, M, K, float(np.float32(max_d2)), p(nq),
                                ctypes.addressof(o), ctypes.addressof(c), p(ws), flags, p(idx), p(dist), p(count), p(eq), st), "pn2_grid_knn")
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return dict(idx=host(idx), dist=host(dist), count=host(count), err_build=None if eb is None else int(eb.item()),
                err_query=None if eq is None else int(eq.item()))


def assert_equals_reference(got, ref, K=None):
    """The written rows equal the reference (its first K columns: the first K of one ordering), the others keep their patterns."""
    w = ref["written"]
    K = got["idx"].shape[2] if K is None else K
    assert np.array_equal(got["idx"][w], ref["idx"][w][:, :K])
    assert (got["idx"][~w] == IDX_FILL).all()
    if got["dist"] is not None:
        assert np.array_equal(got["dist"][w].view(np.uint32), ref["dist"][w][:, :K].view(np.uint32))
        assert (got["dist"][~w] == np.float32(DIST_FILL)).all()
    if got["count"] is not None:
        assert np.array_equal(got["count"][w], ref["count"][w]) and (got["count"][~w] == COUNT_FILL).all()
    if got["err_build"] is not None:
        assert got["err_build"] == ref["err_build"] and got["err_query"] == ref["err_query"]


KS = (1, 3, 4, 5, 16, 17, 32)
_lattice_cache = {}


def lattice_case(N, M, radius):
    """(query, cand, max_d2, the reference at K = 32): computed once, shared, never written to."""
    key = (N, M, radius)
    if key not in _lattice_cache:
        rng = np.random.default_rng(1000 * N + M)
        cand, query = lattice(rng, 2, M), lattice(rng, 2, N)
        m = np.float32(radius ** 2)
        ref = R.grid_knn(query, cand, 32, m, 0.0, R.default_cell(m))
        for v in (query, cand) + tuple(v for v in ref.values() if isinstance(v, np.ndarray)):
            v.setflags(write=False)
        _lattice_cache[key] = (query, cand, m, ref)
    return _lattice_cache[key]


@pytest.mark.parametrize("radius", [0.25, 0.5, 1.0, 2.0])
@pytest.mark.parametrize("N,M", [(257, 33), (300, 1023), (513, 2500)])
def test_lattice_clouds_equal_the_reference(dev, N, M, radius):
    query, cand, m, ref = lattice_case(N, M, radius)
    for K in KS:
        assert_equals_reference(grid_search(dev, cand, query, K, m), ref, K)
    if radius == 2.0 and M == 2500:
        assert ref["count"].max() > 256                            # cell walks cross 64 and 256 rows
    if radius == 0.25 and M == 2500:
        assert 2 < ref["count"].mean() < 20


@pytest.mark.parametrize("N,M", [(257, 33), (300, 1023)])
def test_lattice_result_equals_knn_point_with_the_cut_applied(dev, N, M):
    """On the lattice every float32 operation of either distance form is exact, so the two searches see the same numbers."""
    for radius in (0.25, 1.0):
        query, cand, m, ref = lattice_case(N, M, radius)
        for K in (1, 5, 16, 32):
            idx, dist = U.knn_point(K, cu(cand, dev), cu(query, dev), return_dist=True)
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
            cut = dist > m
            idx[cut], dist[cut] = M, np.inf
            got = grid_search(dev, cand, query, K, m)
            assert np.array_equal(got["idx"], idx) and np.array_equal(got["dist"].view(np.uint32), dist.view(np.uint32))


def test_propagate_labels_grid_equals_brute(dev):
    rng = np.random.default_rng(5)
    B, N, M = 2, 300, 1023
    cand, query = lattice(rng, B, M), lattice(rng, B, N)
    cand[:, 500:700] = cand[:, 100:300]                            # duplicated candidates: each copy votes
    labels = rng.integers(0, 6, (B, M)).astype(np.int64)
    nq, nc = np.int64([300, 211]), np.int64([1023, 640])
    for k, max_dist in ((5, 0.25), (5, 1.0), (9, 0.5)):
        args = (cu(query, dev), cu(cand, dev), cu(labels, dev))
        kw = dict(k=k, max_dist=max_dist, fill=-4, n_query=cu(nq, dev), n_cand=cu(nc, dev))
        brute = U.propagate_labels(*args, **kw).cpu().numpy()
        grid = U.propagate_labels(*args, search="grid", **kw).cpu().numpy()
        assert np.array_equal(brute, grid)
        assert (grid[1, 211:] == -4).all() and len(np.unique(grid[0])) > 3
    with pytest.raises(ValueError):
        U.propagate_labels(*args, k=5, search="grid")


def ends_case():
    """A 2^-10 lattice at scan scale (|p| < 128, every coordinate a multiple of 2^-10), pitch 4, on a grid whose ENDS run through it:
    the radius is one lattice step, the origin is chosen so that x in [3, 3 + cell) is cell -2^20 (x < 3 lies outside) and
    y in [-5 - cell, -5) is cell 2^20 - 1 (y >= -5 lies outside)."""
    rng = np.random.default_rng(21)
    M, s = 700, 2.0 ** -10
    m = np.float32(s * s)
    cell = R.default_cell(m)
    origin = (3.0 + 1048576.0 * cell, -5.0 - 1048576.0 * cell, 100.0)
    pts = np.empty((2, M, 4), np.float32)
    pts[0, :, 0] = 3.0 + s * rng.integers(-2, 4, M)
    pts[0, :, 1] = -5.0 + s * rng.integers(-4, 2, M)
    pts[0, :, 2] = 100.0 + s * rng.integers(-3, 3, M)
    pts[0, :, 3] = rng.random(M)                                   # (the fourth column is not a coordinate)
    pts[1] = pts[0]                                                # the same coordinates in a second cloud
    return pts, m, cell, origin


def test_grid_ends_error_bits_and_clouds_apart(dev):
    pts, m, cell, origin = ends_case()
    M = pts.shape[1]
    q, valid = R.cells(pts[0], origin, cell)
    assert (q[valid][:, 0] == -1048576).any() and (q[valid][:, 1] == 1048575).any() and 50 < (~valid).sum() < M - 50
    n_cand = np.int64([M, M // 2])
    for K in (4, 16):
        ref = R.grid_knn(None, pts, K, m, origin, cell, n_cand=n_cand)
        assert ref["err_build"] == R.ERR_CAND and ref["err_query"] == R.ERR_QUERY
        # neighbours across the grid's end are not neighbours: brute force would have returned some
        assert not np.array_equal(ref["idx"][0], R.brute_knn(None, pts, K, m, n_cand=n_cand)["idx"][0])
        # two clouds with identical coordinates share nothing: the second one indexes half of its rows and finds only those
        assert (ref["idx"][1][ref["written"][1]] < M // 2).sum() > 0 and ((ref["idx"][1] >= M // 2) & (ref["idx"][1] < M)).sum() == 0
        for flags in (0, _lib.GRID_VISIT_SORTED):
            got = grid_search(dev, pts, None, K, m, origin, cell, n_cand=n_cand, flags=flags)
            assert_equals_reference(got, ref)
            assert (got["count"][0][~valid] == 0).all() and (got["idx"][0][~valid] == M).all()
        qref = R.grid_knn(pts[:, :300], pts, K, m, origin, cell, n_cand=n_cand)
        assert_equals_reference(grid_search(dev, pts, pts[:, :300], K, m, origin, cell, n_cand=n_cand), qref)


def test_planted_rows(dev):
    K = 5
    m = np.float32(0.25)
    rng = np.random.default_rng(8)
    cand = np.full((1, 64, 3), 50.0, np.float32) + rng.integers(0, 8, (1, 64, 3)).astype(np.float32)       # far from everything planted
    copies = rng.permutation(64)[:K + 3]
    cand[0, copies] = (1.25, 2.5, -3.0)                            # K + 3 copies of query 0
    ring = rng.permutation(np.setdiff1d(np.arange(64), copies))[:6]      # six candidates at one distance from query 1, in shuffled rows
    for j, d in zip(ring, [(0.25, 0, 0), (-0.25, 0, 0), (0, 0.25, 0), (0, -0.25, 0), (0, 0, 0.25), (0, 0, -0.25)]):
        cand[0, j] = np.float32([-7.0, 9.0, 4.0]) + np.float32(d)
    rest = np.setdiff1d(np.arange(64), np.concatenate([copies, ring]))
    cand[0, rest[0]] = (20.0, 20.0, 20.0)                          # a valid candidate ...
    cand[0, rest[1]] = (20.0, np.nan, 20.0)                        # ... next to a NaN one
    query = np.float32([[[1.25, 2.5, -3.0], [-7.0, 9.0, 4.0], [-30.0, -30.0, -30.0], [np.nan, 0.0, 0.0], [20.0, 20.0, 20.125]]])
    ref = R.grid_knn(query, cand, K, m, 0.0, R.default_cell(m))
    got = grid_search(dev, cand, query, K, m)
    assert_equals_reference(got, ref)
    assert got["idx"][0, 0].tolist() == sorted(copies)[:K] and got["count"][0, 0] == K + 3 and (got["dist"][0, 0] == 0).all()
    assert got["idx"][0, 1].tolist() == sorted(ring)[:K] and got["count"][0, 1] == 6
    assert (got["idx"][0, 2] == 64).all() and np.isinf(got["dist"][0, 2]).all() and got["count"][0, 2] == 0       # 27 empty cells
    assert (got["idx"][0, 3] == 64).all() and got["count"][0, 3] == 0                                            # a NaN query
    assert got["idx"][0, 4].tolist() == [rest[0]] + [64] * (K - 1) and got["count"][0, 4] == 1
    assert got["err_build"] == R.ERR_CAND and got["err_query"] == R.ERR_QUERY


def scan_cloud(rng, B, M, ld=4):
    r = 30.0 * rng.random((B, M)) ** 2 + 0.5
    a = 2 * np.pi * rng.random((B, M))
    pts = rng.random((B, M, ld)).astype(np.float32)
    pts[..., 0], pts[..., 1], pts[..., 2] = r * np.cos(a), r * np.sin(a), 3 * rng.random((B, M)) - 1.5
    return pts


def test_self_search_both_visit_orders_and_two_runs_are_byte_identical(dev):
    rng = np.random.default_rng(12)
    B, M, K = 2, 3000, 16
    pts = scan_cloud(rng, B, M)
    pts[0, 17, 1] = np.inf                                         # an invalid row is written too: empty
    m = np.float32(1.0)
    n_cand = np.int64([M, 1234])
    ref = R.grid_knn(None, pts, K, m, 0.0, R.default_cell(m), n_cand=n_cand)
    assert ref["written"][1].sum() == 1234 and (ref["idx"][0, :, 0] == np.arange(M))[np.arange(M) != 17].all()
    runs = [grid_search(dev, pts, None, K, m, n_cand=n_cand, flags=f) for f in (0, _lib.GRID_VISIT_SORTED, 0, _lib.GRID_VISIT_SORTED)]
    for got in runs:
        assert_equals_reference(got, ref)                          # (every row below the count is written, none beyond)
        for k in ("idx", "dist", "count"):
            assert np.array_equal(got[k].view(np.uint8), runs[0][k].view(np.uint8))
    assert (runs[0]["idx"][0, 17] == M).all() and runs[0]["count"][0, 17] == 0


# pn2_grid_build scans the populations of the table's tiles (1 024 slots each; the table has the power of two at or above 2 M slots) 64
# at a time with a carry.  The largest M elsewhere in the suite gives 8 tiles.  Here: 16 and 64 tiles (one step), 128 (two steps: the
# carry is used) and 256 (four steps: a carry that is assigned and not added to would show); tests/test_tile_seams_cpu.py restates the
# capacity rule and the tile counts.  The workspace holds 0xFF bytes: a slot, a start or a record that is read and was not written
# is -1 or NaN.
DISC_SIZES = [(257, 8192), (257, 32768), (257, 32769), (129, 65537)]             # (N, M)
DISC_RADIUS = 0.3
_disc_cache = {}


def disc_case(N, M):
    """(query, cand, n_cand, max_d2, the reference at K = 32) on R.disc_cloud: B = 2, ld = 4, the queries N of each cloud's candidates
    moved by 0.01, the second cloud indexing two thirds of its rows.  Computed once, shared, never written to."""
    if (N, M) not in _disc_cache:
        rng = np.random.default_rng(M)
        cand = R.disc_cloud(rng, 2, M)
        query = np.stack([cand[b, rng.choice(M, N, replace=False)] for b in range(2)]) + np.float32(0.01)
        n_cand = np.int64([M, M - M // 3])
        m = np.float32(DISC_RADIUS ** 2)
        ref = R.grid_knn(query, cand, 32, m, 0.0, R.default_cell(m), n_cand=n_cand)
        for v in (query, cand, n_cand) + tuple(v for v in ref.values() if isinstance(v, np.ndarray)):
            v.setflags(write=False)
        _disc_cache[(N, M)] = (query, cand, n_cand, m, ref)
    return _disc_cache[(N, M)]


@pytest.mark.parametrize("N,M", DISC_SIZES)
def test_disc_clouds_over_16_to_256_slot_tiles(dev, N, M):
    query, cand, n_cand, m, ref = disc_case(N, M)
    assert ref["err_build"] == 0 and (ref["count"][0] >= 1).all() and ref["count"].max() > 2          # (the input: no query is alone)
    for K in (1, 8, 32):
        assert_equals_reference(grid_search(dev, cand, query, K, m, n_cand=n_cand, fill=0xFF), ref, K)


def test_self_search_over_128_slot_tiles_in_both_visit_orders(dev):
    """M = 32 769: every row below the count is written and nothing beyond it, and every 127th row equals the reference of those rows
    given as explicit queries."""
    _, cand, n_cand, m, _ = disc_case(257, 32769)
    M, K = cand.shape[1], 8
    rows = np.arange(0, M, 127)
    ref = R.grid_knn(cand[:, rows], cand, K, m, 0.0, R.default_cell(m), n_cand=n_cand)
    for flags in (0, _lib.GRID_VISIT_SORTED):
        got = grid_search(dev, cand, None, K, m, n_cand=n_cand, flags=flags, fill=0xFF)
        assert got["err_build"] == 0 and got["err_query"] == 0
        for b in range(2):
            n = int(n_cand[b])
            assert (got["idx"][b, :n] != IDX_FILL).all() and (got["dist"][b, :n] != np.float32(DIST_FILL)).all() and (got["count"][b, :n] != COUNT_FILL).all()
            assert (got["idx"][b, n:] == IDX_FILL).all() and (got["dist"][b, n:] == np.float32(DIST_FILL)).all() and (got["count"][b, n:] == COUNT_FILL).all()
            below = rows < n
            assert np.array_equal(got["idx"][b, rows[below]], ref["idx"][b, below])
            assert np.array_equal(got["dist"][b, rows[below]].view(np.uint32), ref["dist"][b, below].view(np.uint32))
            assert np.array_equal(got["count"][b, rows[below]], ref["count"][b, below])
            assert (got["idx"][b, rows[below], 0] == rows[below]).all()            # a row's nearest neighbour is the row itself


def test_device_counts_leave_the_rows_beyond_untouched(dev):
    rng = np.random.default_rng(13)
    B, N, M, K = 2, 700, 1500, 8
    cand, query = scan_cloud(rng, B, M, 3), scan_cloud(rng, B, N, 5)
    m = np.float32(2.25)
    for n_query, n_cand in ((np.int64([700, 0]), np.int64([1500, 1500])), (np.int64([1, 699]), np.int64([33, 0])),
                            (np.int64([900, -5]), np.int64([2000, 7]))):
        ref = R.grid_knn(query, cand, K, m, 0.0, R.default_cell(m), n_query=n_query, n_cand=n_cand)
        assert_equals_reference(grid_search(dev, cand, query, K, m, n_query=n_query, n_cand=n_cand), ref)


def test_optional_outputs_may_be_null_and_refusals_touch_nothing(dev):
    query, cand, m, ref = lattice_case(300, 1023, 0.5)
    assert_equals_reference(grid_search(dev, cand, query, 5, m, want=()), ref, 5)
    assert_equals_reference(grid_search(dev, cand, query, 5, m, want=("count",)), ref, 5)
    lib = _lib.load()
    B, N, M, K = 2, 300, 1023, 5
    o, c = triple(0.0), triple(R.default_cell(m))
    ws = torch.zeros(lib.pn2_grid_workspace_bytes(B, M), device=dev, dtype=torch.uint8)
    idx = torch.full((B, N, 40), IDX_FILL, device=dev, dtype=torch.int64)
    dist = torch.full((B, N, 40), DIST_FILL, device=dev, dtype=torch.float32)
    count = torch.full((B, N), COUNT_FILL, device=dev, dtype=torch.int32)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    dq = cu(query, dev)
    p = _lib.ptr
    call = lambda K=K, N=N, q=p(dq), cell=ctypes.addressof(c), flags=0: lib.pn2_grid_knn(
        q, 3, B, N, M, K, float(m), None, ctypes.addressof(o), cell, p(ws), flags, p(idx), p(dist), p(count), p(err), _lib.stream())
    bad = triple((1.0, 0.0, 1.0))
    assert call(K=33) == _lib.PN2_EUNSUPPORTED and call(K=0) == -1 and call(q=None) == -1 and call(cell=ctypes.addressof(bad)) == -1
    assert call(flags=4) == -1
    assert lib.pn2_grid_build(p(dq), 3, B, N, None, ctypes.addressof(o), ctypes.addressof(bad), p(err), p(ws), _lib.stream()) == -1
    torch.cuda.synchronize()
    assert (idx == IDX_FILL).all() and (dist == DIST_FILL).all() and (count == COUNT_FILL).all() and int(err.item()) == 0
    assert int(ws.max().item()) == 0


def test_front_end_shapes_and_radius_knn(dev):
    query, cand, m, ref = lattice_case(300, 1023, 0.5)
    idx, dist, count = neighbors.radius_knn(cu(query, dev), cu(cand, dev), 5, 0.5, return_dist=True, return_count=True)
    assert idx.shape == (2, 300, 5) and np.array_equal(idx.cpu().numpy(), ref["idx"][:, :, :5])
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), ref["dist"][:, :, :5].view(np.uint32))
    assert np.array_equal(count.cpu().numpy(), ref["count"])
    flat = neighbors.GridIndex(radius=0.5).build(cu(cand[1], dev))
    assert np.array_equal(flat.query(cu(query[1], dev), 5).cpu().numpy(), ref["idx"][1, :, :5])
    own = flat.query_self(3, return_count=True)
    sref = R.grid_knn(None, cand[1:], 3, m, 0.0, R.default_cell(m))
    assert own[0].shape == (1023, 3) and np.array_equal(own[0].cpu().numpy(), sref["idx"][0]) and np.array_equal(own[1].cpu().numpy(), sref["count"][0])
    flat.check()
    with pytest.raises(RuntimeError):
        flat.query_self(33)


def test_graph_replay_on_new_inputs_equals_the_reference(dev):
    """Build plus query and build plus self-search on preallocated buffers, captured once on one stream, replayed after the points
    and both device-side counts changed in place: the NEW inputs' reference, and not a byte allocated."""
    rng = np.random.default_rng(4)
    B, N, M, K = 2, 500, 900, 7
    cases = [(scan_cloud(rng, B, M), scan_cloud(rng, B, N, 3), nc, nq) for nc, nq in
             ((np.int64([900, 311]), np.int64([500, 17])), (np.int64([40, 900]), np.int64([0, 500])), (np.int64([900, 900]), np.int64([499, 1])))]
    index = neighbors.GridIndex(radius=1.5)
    buf, sbuf = index.buffers(M, B=B, N=N, k=K), index.buffers(M, B=B, k=K)
    cand, query = torch.zeros(B, M, 4, device=dev), torch.zeros(B, N, 3, device=dev)
    n_cand, n_query = torch.zeros(B, device=dev, dtype=torch.int64), torch.zeros(B, device=dev, dtype=torch.int64)

    def step():
        index.build(cand, n_cand=n_cand, buffers=buf)
        a = index.query(query, K, n_query=n_query, return_dist=True, return_count=True, buffers=buf)
        index.build(cand, n_cand=n_cand, buffers=sbuf)
        return a, index.query_self(K, return_dist=True, return_count=True, buffers=sbuf)

    def load(case):
        for t, v in zip((cand, query, n_cand, n_query), case):
            t.copy_(cu(v, dev))

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    assert res[0][0] is not None and res[0][0].data_ptr() == buf.idx.data_ptr() and res[1][2] is sbuf.count
    m = np.float32(1.5 ** 2)
    for case in cases[1:] + cases[:1]:
        load(case)
        for b in (buf, sbuf):
            b.idx.fill_(IDX_FILL), b.dist.fill_(DIST_FILL), b.count.fill_(COUNT_FILL)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        for b, q, nq in ((buf, case[1], case[3]), (sbuf, None, None)):
            ref = R.grid_knn(q, case[0], K, m, 0.0, R.default_cell(m), n_query=nq, n_cand=case[2])
            got = dict(idx=b.idx.cpu().numpy(), dist=b.dist.cpu().numpy(), count=b.count.cpu().numpy(), err_build=None, err_query=None)
            assert_equals_reference(got, ref)
            assert int(b.error_flag.item()) == 0


def test_estimate_normals_grid_against_brute_on_the_sphere(dev):
    """The unit sphere of tests/test_normals_gpu.py.  Off a lattice the two distance forms may order near-ties differently, so the
    neighbour SETS are compared first: they agree on at least 99 % of the rows (the fp64 and the difference-form references agree
    on every row of this cloud); where the two lists are the same, normal, cov and count have the same bits."""
    rng = np.random.default_rng(2048)
    M, k, radius = 2048, 16, 0.25
    v = rng.standard_normal((M, 3))
    pts = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    xd = cu(pts, dev)
    m = np.float32(radius ** 2)
    bi, bd = U.knn_point(k, xd[None], xd[None], return_dist=True)
    bi = torch.where(bd > float(m), torch.full_like(bi, M), bi).cpu().numpy()[0]
    gi = neighbors.radius_knn(None, xd, k, radius).cpu().numpy()
    assert np.array_equal(gi, R.grid_knn(None, pts[None], k, m, 0.0, R.default_cell(m))["idx"][0])
    agree = (np.sort(bi, -1) == np.sort(gi, -1)).all(-1)
    print("\nsphere: the neighbour sets agree on %d of %d rows" % (agree.sum(), M))
    assert agree.mean() >= 0.99
    kw = dict(k=k, radius=radius, viewpoint="origin", return_cov=True, return_count=True)
    brute = [t.cpu().numpy() for t in PN.estimate_normals(xd, **kw)]
    grid = [t.cpu().numpy() for t in PN.estimate_normals(xd, search="grid", **kw)]
    same_order = (bi == gi).all(-1)                                # (the covariance is a sum in slot order: same sets in the same order)
    assert same_order.mean() >= 0.99
    for a, b in zip(brute, grid):
        assert np.array_equal(a[same_order].view(np.uint8), b[same_order].view(np.uint8))
    with pytest.raises(ValueError):
        PN.estimate_normals(xd, k=k, search="grid")
    buf = PN.buffers(M, k=k, device=dev, search="grid")
    again = PN.estimate_normals(xd, buffers=buf, search="grid", **kw)
    for a, b in zip(grid, again):
        assert np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))


class _SignStub(torch.nn.Module):
    """A stand-in for the network: [1, 4, n] -> log-probabilities [1, n, 4], class 2 where x > 0 and class 1 elsewhere."""

    def forward(self, x):
        pos = (x[:, 0, :] > 0).unsqueeze(-1)
        return torch.log_softmax(torch.where(pos, x.new_tensor([0.0, 0.0, 9.0, 0.0]), x.new_tensor([0.0, 9.0, 0.0, 0.0])), -1)


def test_label_scan_grid_equals_brute(dev):
    """``FrameSegmenter.label_scan(search="grid")`` on a scan of whole eighths (every float32 distance of either form is exact) with
    equally seeded draws: the labels of ``search="brute"``, row for row, a second call on the kept workspace included."""
    from conftest import golden
    from pointnet12_amd import kitti
    from pointnet12_amd import kitti_view as V
    g = golden("g18_kitti_view.npz")
    rng = np.random.default_rng(21)
    M, n = 3000, 1024
    raw = np.empty((M, 4), np.float32)
    raw[:, 0] = rng.choice([-1, 1], M) * rng.integers(16, 96, M) / 8
    raw[:, 1] = rng.integers(-24, 25, M) / 8
    raw[:, 2] = rng.integers(-8, 9, M) / 8
    raw[:, 3] = rng.integers(0, 100, M) / 100
    words = rng.choice(np.uint32([0, 1, 2, 5]), M, p=[0.1, 0.3, 0.3, 0.3])
    sf = kitti.ScanFilter({0: 0, 1: 1, 2: 2, 5: 3}, "all", x_range=(-11, 11), device=dev)
    lut = cu(np.int32([40, 44, 48, 70]), dev)
    seg = V.FrameSegmenter(_SignStub().to(dev), V.Calibration(g["R"], g["T"], g["P"]), g["colors"], npoints=n)
    raw_d, words_d = cu(raw, dev), cu(words.view(np.int32), dev)
    run = lambda search, max_dist: seg.label_scan(raw_d, words_d, scan_filter=sf, rng=torch.Generator(device=dev).manual_seed(3), k=5,
                                                  max_dist=max_dist, lut=lut, search=search)["scan_labels"].cpu().numpy().copy()
    for max_dist in (1.0, 0.25):
        brute = run("brute", max_dist)
        assert np.array_equal(run("grid", max_dist), brute) and np.array_equal(run("grid", max_dist), brute)
        assert set(np.unique(brute)) >= {0, 44, 48}
    assert int(seg.error_flag.item()) == 0
    with pytest.raises(ValueError):
        run("grid", None)
