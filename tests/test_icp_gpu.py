"""GPU: pn2_icp_step against tests/icp_ref.py at the C ABI.  Correspondences, counts, status and error bits EQUAL the reference;
the sums are the reference's terms in another order and are held to the bound that follows from that alone; the solve and the
update are held to the DEVICE's own sums and x."""
import ctypes

import numpy as np
import pytest
import torch

import grid_knn_ref as R
import icp_ref as I
from geometry_ref import lattice
from pointnet12_amd import _lib, registration

pytestmark = pytest.mark.gpu

F64_FILL, I64_FILL = -123.25, -77           # what outputs hold before a call: what a call must not touch keeps it
IDENTITY = np.eye(3, 4).reshape(12)


def cu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def triple(v):
    return (ctypes.c_double * 3)(*np.broadcast_to(np.asarray(v, np.float64), (3,)))


class Pair:
    """Target clouds on the device with their grid built (pn2_grid_build at the C ABI), and the source clouds."""

    def __init__(self, dev, src, tgt, normals, max_d2, n_src=None, fill=0xA5):
        lib = _lib.load()
        self.dev, self.src_np, self.tgt_np, self.nrm_np, self.max_d2, self.n_src_np = dev, src, tgt, normals, np.float32(max_d2), n_src
        self.B, self.N, self.lds = src.shape
        self.M, self.ldt = tgt.shape[1:]
        self.cell = R.default_cell(self.max_d2)
        self.o, self.c = triple(0.0), triple(self.cell)
        self.src, self.tgt = cu(src, dev), cu(tgt, dev)
        self.nrm = None if normals is None else cu(normals, dev)
        self.n_src = None if n_src is None else cu(np.asarray(n_src, np.int64), dev)
        self.grid = torch.full((lib.pn2_grid_workspace_bytes(self.B, self.M),), fill, device=dev, dtype=torch.uint8)
        self.work = torch.full((lib.pn2_icp_workspace_bytes(self.B, self.N),), fill, device=dev, dtype=torch.uint8)      # (it may hold anything)
        _lib.check(lib.pn2_grid_build(_lib.ptr(self.tgt), self.ldt, self.B, self.M, None, ctypes.addressof(self.o), ctypes.addressof(self.c),
                                      None, _lib.ptr(self.grid), _lib.stream()), "pn2_grid_build")

    def state(self, T, status=None, iters=None):
        """The read-and-written arguments and the prefilled outputs of a step, on the device."""
        B, dev = self.B, self.dev
        return dict(T=cu(np.asarray(T, np.float64).reshape(B, 12), dev),
                    status=cu(np.zeros(B, np.int32) if status is None else np.asarray(status, np.int32), dev),
                    iters=cu(np.zeros(B, np.int32) if iters is None else np.asarray(iters, np.int32), dev),
                    sums=torch.full((B, 28), F64_FILL, device=dev, dtype=torch.float64), x=torch.full((B, 6), F64_FILL, device=dev, dtype=torch.float64),
                    count=torch.full((B,), I64_FILL, device=dev, dtype=torch.int64), corr=torch.full((B, self.N), I64_FILL, device=dev, dtype=torch.int64),
                    err=torch.zeros(1, device=dev, dtype=torch.int32))

    def step(self, st, metric, flags=0, tol_rot=0.0, tol_trans=0.0, corr=True, **over):
        """One pn2_icp_step on the device state ``st`` -> the return code."""
        p = _lib.ptr
        a = dict(src=p(self.src), lds=self.lds, B=self.B, N=self.N, n_src=p(self.n_src), tgt=p(self.tgt), ldt=self.ldt, M=self.M,
                 nrm=p(self.nrm) if metric == I.PLANE else None, ldn=0 if self.nrm is None else self.nrm.shape[2], o=ctypes.addressof(self.o),
                 c=ctypes.addressof(self.c), grid=p(self.grid), max_d2=float(self.max_d2), metric=metric, flags=flags, tol_rot=tol_rot,
                 tol_trans=tol_trans, T=p(st["T"]), sums=p(st["sums"]), count=p(st["count"]), x=p(st["x"]), status=p(st["status"]),
                 iters=p(st["iters"]), corr=p(st["corr"]) if corr else None, err=p(st["err"]), work=p(self.work))
        a.update(over)
        return _lib.load().pn2_icp_step(a["src"], a["lds"], a["B"], a["N"], a["n_src"], a["tgt"], a["ldt"], a["M"], a["nrm"], a["ldn"], a["o"],
                                        a["c"], a["grid"], a["max_d2"], a["metric"], a["flags"], a["tol_rot"], a["tol_trans"], a["T"],
                                        a["sums"], a["count"], a["x"], a["status"], a["iters"], a["corr"], a["err"], a["work"], _lib.stream())

    def reference(self, T, metric, status=None, iters=None, flags=0, tol_rot=0.0, tol_trans=0.0):
        B = self.B
        return I.icp_step(self.src_np, self.tgt_np, self.nrm_np, np.asarray(T, np.float64).reshape(B, 12),
                          np.zeros(B, np.int32) if status is None else status, np.zeros(B, np.int32) if iters is None else iters,
                          self.max_d2, 0.0, self.cell, metric, flags, tol_rot, tol_trans, self.n_src_np)


def host(st):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in st.items()}


def perturbed_planted():
    """The planted transform with 0.01 rad about (3, -1, 2) and (0.004, 0.003, -0.002) put on top."""
    D = I.rotation((3, -1, 2), 0.01)
    return np.concatenate([D @ I.PLANTED_R, (D @ I.PLANTED_T + [0.004, 0.003, -0.002])[:, None]], 1).reshape(12)


_cases = {}


def lattice_case(N, ld, M=1000, seed=None):
    """B = 3 lattice clouds (ties exist), M targets, drawn from ``seed`` (100 N + ld unless given), radius 0.15 (a little above one lattice step of 1/8, so some rows have
    nobody in the ball), cloud 0 from the identity, cloud 1 from the perturbed planted transform with one row fewer, cloud 2 with
    count 0.  Planted: source rows far from every target, a NaN source row, zero and NaN normals.  Host arrays, read-only, once."""
    key = (N, ld, M, seed)
    if key not in _cases:
        rng = np.random.default_rng(100 * N + ld if seed is None else seed)
        B = 3
        src, tgt = np.zeros((B, N, ld), np.float32), np.zeros((B, M, ld), np.float32)
        src[..., :3], tgt[..., :3] = lattice(rng, B, N), lattice(rng, B, M)
        src[..., 3:], tgt[..., 3:] = rng.random((B, N, ld - 3)), rng.random((B, M, ld - 3))          # (not coordinates)
        if N > 8:
            src[0, 3, :3] = (40.0, 40.0, 40.0)                     # 27 empty cells
            src[0, N - 2, :3] = (1.03, 0.875, 0.875)                  # cells with candidates, none within the ball
            src[1, 5, 1] = np.nan                                  # PN2_ICP_ERR_QUERY
        v = rng.standard_normal((B, M, 3))
        normals = np.zeros((B, M, 6), np.float32)                  # [.,6] rows: the normal in columns 0..2
        normals[..., :3] = v / np.linalg.norm(v, axis=-1, keepdims=True)
        normals[..., 3:] = 9.0
        normals[:, 7::31, :3] = 0.0                                # PN2_PCA_ERR_FEW's normal
        normals[:, 11::29, 2] = np.nan
        n_src = np.int64([N, N - 1, 0])
        T = np.stack([IDENTITY, perturbed_planted(), IDENTITY])
        for a in (src, tgt, normals, n_src, T):
            a.setflags(write=False)
        _cases[key] = (src, tgt, normals, n_src, T)
    return _cases[key]


def assert_step_matches(got, ref, T_in, metric):
    """One step's device outputs against the reference (see the module docstring); frozen clouds keep their patterns."""
    w, t = ref["corr"] >= 0, ref["touched"]
    assert np.array_equal(got["corr"][w], ref["corr"][w]) and (got["corr"][~w] == I64_FILL).all()
    assert np.array_equal(got["count"][t], ref["count"][t]) and (got["count"][~t] == I64_FILL).all()
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["iters"], ref["iters"]) and int(got["err"][0]) == ref["err"]
    for b in np.flatnonzero(t):
        # the same terms in another order: |difference| <= count * 2^-52 * sum |term|
        count = float(ref["count"][b])
        bound = count * 2.0 ** -52 * ref["abs_sums"][b]
        diff = np.abs(got["sums"][b] - ref["sums"][b])
        print("cloud %d: count %d, worst sums difference / bound = %.3g" % (b, count, (diff / np.maximum(bound, 1e-300)).max()))
        assert (diff <= bound).all()
        if ref["status"][b] & I.SINGULAR:
            assert (got["x"][b] == 0).all() and np.array_equal(got["T"][b], T_in[b])
            continue
        A, rhs, _ = I.matrices(got["sums"][b])
        x = got["x"][b]
        res = np.abs(A @ x + rhs).max()
        assert res <= 2.0 ** -44 * (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(rhs).max())
        want, _, _ = I.update(T_in[b], x)
        assert (np.abs(got["T"][b] - want) <= 2.0 ** -49 * (1.0 + np.abs(T_in[b].reshape(3, 4)[:, 3]).max() + np.abs(x[3:]).max())).all()
        # The reference's own T: A and b differ entry by entry by at most count * 2^-52 of the sums of magnitudes (above), which are at
        # most sqrt(A_kk A_ll) -- normwise 6 * count * 2^-52 -- so x differs by about cond(A) times that, relatively, and an entry of
        # T by that times the points' reach (|p| <= 2.5 here); 32 covers the 6, the reach and the solve's own rounding.
        tol = 32.0 * np.linalg.cond(A) * count * 2.0 ** -52 * np.abs(ref["x"][b]).max() + 2.0 ** -48
        assert np.abs(got["T"][b] - ref["T"][b]).max() <= tol


@pytest.mark.parametrize("ld", [3, 4])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_single_steps_equal_the_reference(dev, N, ld):
    src, tgt, normals, n_src, T = lattice_case(N, ld)
    pair = Pair(dev, src, tgt, normals, 0.15 ** 2, n_src)
    for metric in (I.PLANE, I.POINT):
        st = pair.state(T)
        assert pair.step(st, metric) == 0
        got, ref = host(st), pair.reference(T, metric)
        assert_step_matches(got, ref, T, metric)
        assert got["status"][2] == I.SINGULAR and got["count"][2] == 0 and (got["corr"][2] == I64_FILL).all()
        if N > 8:
            assert got["corr"][0, 3] == 1000 and got["corr"][0, N - 2] == 1000 and got["corr"][1, 5] == 1000 and got["err"][0] & I.ERR_QUERY
            assert got["corr"][1, N - 1] == I64_FILL and 0 < got["count"][0] < N - 2
        if N >= 1023 and metric == I.PLANE:
            matched = ref["corr"][0][ref["corr"][0] < 1000]
            assert (normals[0, matched, 0] == 0).any() and np.isnan(normals[0, matched, 2]).any()     # rows that name j and take no part
            assert got["count"][0] < len(matched)


# Past the first trip of the finish kernel's loop over tiles (thread (k, c) adds word k of tiles c, c + 8, c + 16, ...): 8 tiles (one per
# chunk), 9 (chunk 0 takes two trips, the last tile holds one row) and 17 (three trips).  The device-side counts: cloud 1 ends exactly
# on a tile boundary with whole tiles of the launch beyond it, cloud 2 ends inside a tile.  The same counts serve the plane and the
# correspondence tests; tests/test_tile_seams_cpu.py shows on the reference that a tile lost from these cases cannot pass.
SEAM_COUNTS = {8192: (8192, 4096, 5000), 8193: (8193, 8192, 5000), 16385: (16385, 8192, 9000)}
SEAM_M = 300                                                       # (the reference costs N x M)
SEAM_SEEDS = {8192: 1, 8193: 1, 16385: 4}                         # chosen on the reference: see ``seam_case``


def seam_case(N):
    """``lattice_case(N, 3)`` with 300 targets, the counts above, and a seed for which (on the reference alone) no cloud is singular
    and the LAST row of cloud 0 -- at N = 1024 t + 1 a tile of its own -- takes part under both metrics."""
    src, tgt, normals, _, T = lattice_case(N, 3, SEAM_M, SEAM_SEEDS[N])
    return src, tgt, normals, np.int64(SEAM_COUNTS[N]), T


@pytest.mark.parametrize("N", sorted(SEAM_COUNTS))
def test_single_steps_past_the_first_trip_over_the_tiles(dev, N):
    """The workspace holds 0xFF bytes (NaN as a double): a partial that is read and was not written poisons every sum."""
    src, tgt, normals, n_src, T = seam_case(N)
    pair = Pair(dev, src, tgt, normals, 0.15 ** 2, n_src, fill=0xFF)
    for metric in (I.PLANE, I.POINT):
        st = pair.state(T)
        assert pair.step(st, metric) == 0
        got, ref = host(st), pair.reference(T, metric)
        assert (ref["status"] == 0).all() and (ref["count"] > n_src // 4).all() and ref["corr"][0, N - 1] < SEAM_M      # (the input's conditions)
        assert_step_matches(got, ref, T, metric)
        for b in range(3):
            assert (got["corr"][b, :n_src[b]] != I64_FILL).all() and (got["corr"][b, n_src[b]:] == I64_FILL).all()


def test_k1_walk_over_a_table_of_128_tiles(dev):
    """257 source rows against 32 769 targets on a disc: the target's slot table has 131 072 slots, 128 tiles of 1 024, so the scan of
    the tile populations carries across 64 tiles once, and the K = 1 walk reads cell starts that the carry produced."""
    rng = np.random.default_rng(32769)
    B, N, M = 2, 257, 32769
    tgt = R.disc_cloud(rng, B, M)
    src = np.stack([tgt[b, rng.choice(M, N, replace=False), :3] for b in range(B)]) + np.float32(0.01)
    v = rng.standard_normal((B, M, 3))
    normals = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    D = I.rotation((3, -1, 2), 0.002)                              # (0.024 at the rim of the disc: well inside the ball of 0.3)
    T = np.stack([IDENTITY, np.concatenate([D, np.array([[0.004], [0.003], [-0.002]])], 1).reshape(12)])
    n_src = np.int64([N, 200])
    pair = Pair(dev, src, tgt, normals, 0.3 ** 2, n_src, fill=0xFF)
    for metric in (I.PLANE, I.POINT):
        st = pair.state(T)
        assert pair.step(st, metric) == 0
        got, ref = host(st), pair.reference(T, metric)
        assert (ref["status"] == 0).all() and ref["err"] == 0 and np.array_equal(ref["count"], n_src)       # every row finds somebody
        assert_step_matches(got, ref, T, metric)
        assert (got["corr"][1, 200:] == I64_FILL).all()


def test_frozen_eval_only_and_refusals(dev):
    src, tgt, normals, n_src, T = lattice_case(1025, 4)
    pair = Pair(dev, src, tgt, normals, 0.15 ** 2, np.int64([1025, 1025, 1025]))
    status, iters = np.int32([I.CONVERGED, 0, I.SINGULAR]), np.int32([4, 2, 9])
    st = pair.state(T, status, iters)
    assert pair.step(st, I.PLANE) == 0
    got, ref = host(st), pair.reference(T, I.PLANE, status, iters)
    assert_step_matches(got, ref, T, I.PLANE)
    for b in (0, 2):                                               # frozen: nothing of theirs is touched
        assert (got["sums"][b] == F64_FILL).all() and (got["x"][b] == F64_FILL).all() and got["count"][b] == I64_FILL
        assert (got["corr"][b] == I64_FILL).all() and np.array_equal(got["T"][b], T[b]) and got["iters"][b] == iters[b] and got["status"][b] == status[b]
    assert got["iters"][1] == 3 and got["count"][1] > 6
    # EVAL_ONLY ignores the freeze and writes sums / count / corr only
    st = pair.state(T, status, iters)
    assert pair.step(st, I.POINT, flags=I.EVAL_ONLY) == 0
    got, ref = host(st), pair.reference(T, I.POINT, status, iters, flags=I.EVAL_ONLY)
    assert np.array_equal(got["corr"], ref["corr"]) and np.array_equal(got["count"], ref["count"]) and ref["touched"].all()
    assert (np.abs(got["sums"] - ref["sums"]) <= ref["count"][:, None] * 2.0 ** -52 * ref["abs_sums"]).all()
    assert (got["x"] == F64_FILL).all() and np.array_equal(got["T"], T) and np.array_equal(got["status"], status) and np.array_equal(got["iters"], iters)
    st2 = pair.state(T, status, iters)
    assert pair.step(st2, I.POINT, flags=I.EVAL_ONLY, corr=False, x=None, status=None, iters=None, err=None) == 0      # optional pointers
    assert np.array_equal(host(st2)["sums"].view(np.uint8), got["sums"].view(np.uint8)) and (host(st2)["corr"] == I64_FILL).all()
    # every refusal leaves every output as it was
    st = pair.state(T)
    bad_cell = triple((1.0, 0.0, 1.0))
    refusals = [dict(src=None), dict(tgt=None), dict(T=None), dict(sums=None), dict(count=None), dict(x=None), dict(status=None), dict(iters=None),
                dict(work=None), dict(grid=None), dict(o=None), dict(c=ctypes.addressof(bad_cell)), dict(lds=2), dict(lds=17), dict(ldt=2),
                dict(ldt=17), dict(ldn=2), dict(ldn=17), dict(nrm=None), dict(B=0), dict(B=65536), dict(N=0), dict(M=0), dict(metric=2),
                dict(metric=-1), dict(flags=2), dict(tol_rot=-1.0), dict(tol_trans=float("inf")), dict(tol_rot=float("nan"))]
    for over in refusals:
        over = dict(over)
        assert pair.step(st, over.pop("metric", I.PLANE), **over) == -1, over
    assert _lib.load().pn2_icp_workspace_bytes(0, 5) == -1 and _lib.load().pn2_icp_workspace_bytes(1, 0) == -1
    got = host(st)
    assert (got["sums"] == F64_FILL).all() and (got["x"] == F64_FILL).all() and (got["count"] == I64_FILL).all() and (got["corr"] == I64_FILL).all()
    assert np.array_equal(got["T"], T) and (got["status"] == 0).all() and (got["iters"] == 0).all() and got["err"][0] == 0


def test_a_transform_that_is_not_finite_is_flagged_and_left_alone(dev):
    src, tgt, normals, n_src, T = lattice_case(65, 3)
    pair = Pair(dev, src, tgt, normals, 0.15 ** 2, n_src)
    T = T.copy()
    T[0, 7] = np.nan                                               # cloud 0: every row becomes an invalid query, the cloud singular
    st = pair.state(T)
    assert pair.step(st, I.PLANE) == 0
    got, ref = host(st), pair.reference(T, I.PLANE)
    assert ref["err"] == I.ERR_QUERY | I.ERR_NONFINITE | I.ERR_SINGULAR and ref["status"].tolist() == [I.SINGULAR, 0, I.SINGULAR]
    assert np.array_equal(got["status"], ref["status"]) and int(got["err"][0]) == ref["err"] and np.array_equal(got["iters"], [0, 1, 0])
    assert np.array_equal(got["T"][0].view(np.uint64), T[0].view(np.uint64)) and (got["x"][0] == 0).all() and got["count"][0] == 0
    assert (got["corr"][0] == 1000).all() and (got["sums"][0] == 0).all()


def sheets(dev, B=1):
    src, tgt, normals = I.sheets_pair()
    rep = lambda a: np.ascontiguousarray(np.repeat(a, B, 0))
    return Pair(dev, rep(src), rep(tgt), rep(normals), I.SHEETS_MAX_DIST ** 2)


def abi_loop(pair, T, metric, iterations=30, tol_rot=1e-6, tol_trans=1e-6 * I.SHEETS_MAX_DIST):
    st = pair.state(T)
    for _ in range(iterations):
        assert pair.step(st, metric, tol_rot=tol_rot, tol_trans=tol_trans) == 0
    return st


def test_thirty_steps_twice_are_byte_identical(dev):
    pair = sheets(dev, B=2)
    T = np.stack([IDENTITY, perturbed_planted()])
    for metric in (I.PLANE, I.POINT):
        runs = [host(abi_loop(pair, T, metric, tol_rot=0.0, tol_trans=0.0)) for _ in range(2)]       # (tolerance 0: all 30 steps walk)
        assert (runs[0]["iters"] == 30).all()
        for k in ("T", "sums", "corr", "x", "count"):
            assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), k
        Rm = runs[0]["T"].reshape(2, 3, 4)[:, :, :3]
        assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() <= 30 * 2.0 ** -50


@pytest.mark.parametrize("metric", [I.PLANE, I.POINT])
def test_end_to_end_recovers_the_planted_transform(dev, metric):
    ref, e_ref, cond = I.sheets_reference(metric)
    got = host(abi_loop(sheets(dev), IDENTITY[None], metric))
    e = np.abs(got["T"][0] - I.PLANTED).max()
    bound = max(16 * e_ref, cond * 2.0 ** -50)
    print("\nmetric %d: |T - T*| = %.3g, e_ref = %.3g (ratio %.3g), cond(A) = %.3g, bound %.3g, %d iterations (reference %d)" %
          (metric, e, e_ref, e / e_ref, cond, bound, got["iters"][0], ref["iters"][0]))
    assert got["status"][0] == I.CONVERGED and got["iters"][0] <= 30
    assert got["status"][0] == ref["status"][0] and got["iters"][0] == ref["iters"][0]
    assert e <= bound


def result_bytes(res):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy().copy() for t in res]


def test_python_layer_agrees_with_the_abi_loop_and_the_reference(dev):
    src, tgt, normals = I.sheets_pair()
    s, t, n = cu(src[0], dev), cu(tgt[0], dev), cu(normals[0], dev)
    for name, metric in (("plane", I.PLANE), ("point", I.POINT)):
        want = host(abi_loop(sheets(dev), IDENTITY[None], metric))
        res = registration.icp(s, t, I.SHEETS_MAX_DIST, metric=name, target_normals=n, return_corr=True)
        T, fitness, rmse, iters, status, corr = result_bytes(res)
        assert T.shape == (4, 4) and np.array_equal(T[:3].reshape(12), want["T"][0]) and np.array_equal(T[3], [0, 0, 0, 1])
        assert iters == want["iters"][0] and status == want["status"][0] == I.CONVERGED
        m = np.float32(I.SHEETS_MAX_DIST ** 2)
        ev = I.icp_step(src, tgt, None, T[:3].reshape(1, 12), np.zeros(1, np.int32), np.zeros(1, np.int32), m, 0.0, R.default_cell(m), I.POINT,
                        flags=I.EVAL_ONLY)                         # the reference's evaluation AT THE DEVICE'S transform
        assert np.array_equal(corr, ev["corr"][0]) and fitness == ev["count"][0] / 1024 == 1.0
        r_ref = np.sqrt(ev["sums"][0, 27] / ev["count"][0])
        assert abs(rmse - r_ref) <= (1024 * 2.0 ** -52 + 2.0 ** -51) * r_ref            # E within its sums bound (every term >= 0), one sqrt
        f2, r2 = registration.evaluate(s, t, res.transform, I.SHEETS_MAX_DIST)
        assert np.array_equal(result_bytes([f2, r2]), [fitness, rmse])
        f3, r3, c3 = registration.evaluate(s[None], t[None], torch.eye(4, device=dev, dtype=torch.float64), 0.01, return_corr=True)
        e0 = I.icp_step(src, tgt, None, IDENTITY[None], np.zeros(1, np.int32), np.zeros(1, np.int32), np.float32(0.01 ** 2), 0.0,
                        R.default_cell(np.float32(0.01 ** 2)), I.POINT, flags=I.EVAL_ONLY)
        assert np.array_equal(c3.cpu().numpy(), e0["corr"]) and float(f3[0]) == e0["count"][0] / 1024 < 0.2
    # nobody within reach: fitness 0 and rmse +0.0
    far = registration.icp(s + 100.0, t, 0.5, metric="point", iterations=2)
    assert float(far.fitness) == 0.0 and float(far.rmse) == 0.0 and not np.signbit(float(far.rmse)) and int(far.status) == I.SINGULAR
    assert int(far.iterations) == 0 and far.corr is None
    # the default normals (estimated from the target) lead to the same place: at the planted transform every residual is zero
    # whatever the normals, so the fixed point is the same and only the float32 rounding of the source (2^-24 of coordinates up
    # to 2.5, 1.5e-7) is seen through another, still well-conditioned, system
    est = registration.icp(s, t, I.SHEETS_MAX_DIST)
    e = np.abs(est.transform.cpu().numpy()[:3].reshape(12) - I.PLANTED).max()
    print("\ndefault normals: |T - T*| = %.3g after %d iterations" % (e, int(est.iterations)))
    assert int(est.status) == I.CONVERGED and e <= 1e-6
    # transform_points: numpy's bits
    pts = cu(src, dev)
    Tm = cu(perturbed_planted().reshape(3, 4), dev)
    want = I.transform(perturbed_planted(), src[0]).astype(np.float32)
    assert np.array_equal(registration.transform_points(pts, Tm).cpu().numpy()[0].view(np.uint32), want.view(np.uint32))
    out = torch.full((1024, 5), 7.0, device=dev)
    assert registration.transform_points(pts[0], Tm, out=out) is out
    assert np.array_equal(out.cpu().numpy()[:, :3].view(np.uint32), want.view(np.uint32)) and (out[:, 3:] == 7.0).all()


def test_graph_replay_on_new_points_init_and_counts_equals_eager(dev):
    rng = np.random.default_rng(9)
    src0, tgt0, _ = I.sheets_pair()
    B, N, M = 2, 1024, 2048
    shift = np.float32([0.25, -0.125, 0.5])
    cases = []
    for k in range(3):
        tgt = np.stack([tgt0[0], tgt0[0][::-1] + shift * k])
        src = np.stack([src0[0], src0[0][::-1] + shift * k])
        src[0] = src[0][rng.permutation(N)]
        init = np.stack([I.rotation((0, 0, 1), 0.004 * k) @ np.eye(3, 4), np.eye(3, 4)])
        cases.append((src.astype(np.float32), tgt.astype(np.float32), init, np.int64([N - 100 * k, N // (k + 1)]), np.int64([M, M - 7 * k])))
    src, tgt = torch.zeros(B, N, 3, device=dev), torch.zeros(B, M, 3, device=dev)
    init = torch.zeros(B, 3, 4, device=dev, dtype=torch.float64)
    n_source, n_target = torch.zeros(B, device=dev, dtype=torch.int64), torch.zeros(B, device=dev, dtype=torch.int64)
    buf, eager_buf = registration.buffers(N, M, B, device=dev), registration.buffers(N, M, B, device=dev)

    def run(b):
        return registration.icp(src, tgt, I.SHEETS_MAX_DIST, init=init, iterations=8, n_source=n_source, n_target=n_target, return_corr=True, buffers=b)

    def load(case):
        for t, v in zip((src, tgt, init, n_source, n_target), case):
            t.copy_(cu(v, dev))

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run(buf)
    assert res.transform.data_ptr() == buf.transform.data_ptr()
    for case in cases[1:] + cases[:1]:
        load(case)
        buf.corr.fill_(I64_FILL), eager_buf.corr.fill_(I64_FILL)
        graph.replay()
        got = result_bytes(res)
        want = result_bytes(run(eager_buf))
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert (got[4] & I.SINGULAR == 0).all() and (got[1] > 0.9).all() and int(buf.error_flag.item()) == 0
        assert (got[5][1, int(case[3][1]):] == I64_FILL).all()
