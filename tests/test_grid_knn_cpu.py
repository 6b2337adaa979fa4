"""CPU: the grid kNN rule (tests/grid_knn_ref.py) equals brute force when the cell carries its margin and does NOT without it; the
refusals of pn2_grid_build / pn2_grid_knn / pn2_grid_workspace_bytes need no GPU; the lattice cases of tests/test_grid_knn_gpu.py
hold what they are meant to hold; the generated code of csrc/grid_knn.hip uses no scratch."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import grid_knn_ref as R
from conftest import ROOT
from geometry_ref import lattice
from pointnet12_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
SAME = ("idx", "dist", "count")


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if k == "dist" else a[k], b[k].view(np.uint32) if k == "dist" else b[k]) for k in SAME)


def step(x, n):
    """x moved n float32 ulps (towards +inf for n > 0)."""
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf))
    return x


def border_pairs(radius, margin, kmax=3000):
    """Adversarial pairs along x: queries within two ulps of the cell borders k * cell, |k| <= kmax, and for each a candidate at
    q +- t with t within three ulps of the cut sqrt(max_d2) (y = z = 0).  -> q, p float32 [n], in_ball, outside_27 bool [n]."""
    m = np.float32(radius ** 2)
    cell = np.sqrt(np.float64(m)) * (1.0 + margin)
    q0 = (np.arange(-kmax, kmax + 1) * cell).astype(np.float32)
    t0 = np.float32(np.sqrt(np.float64(m)))
    qs, ps = [], []
    for dq in range(-2, 3):
        q = step(q0, dq)
        for sign in (-1.0, 1.0):
            for j in range(-3, 4):
                qs.append(q)
                ps.append(q + np.float32(sign) * step(np.full_like(q, t0), j))
    q, p = np.concatenate(qs), np.concatenate(ps)
    t = q - p
    in_ball = t * t <= m                                  # (y = z = 0: the two fmaf add exact zeros)
    outside = np.abs(np.floor(q.astype(np.float64) / cell) - np.floor(p.astype(np.float64) / cell)) > 1
    return q, p, in_ball, outside


@pytest.mark.parametrize("radius", [0.3, 0.5, 1.0])
def test_the_margin_keeps_every_in_ball_pair_inside_the_27_cells_and_its_absence_does_not(radius):
    q, p, in_ball, outside = border_pairs(radius, 2.0 ** -20)
    assert in_ball.sum() > 100000 and (~in_ball).sum() > 300            # both sides of the cut are populated
    assert (in_ball & outside).sum() == 0
    q, p, in_ball, outside = border_pairs(radius, 0.0)
    bad = np.flatnonzero(in_ball & outside)
    assert bad.size > 0                                                 # without the margin the pruning loses pairs: the check can fail
    # ... and the loss shows in the statement itself: a cloud of the offending pairs (and as many harmless ones)
    pick = np.concatenate([bad, np.arange(0, q.size, q.size // 200)])
    xyz = lambda x: np.stack([x, np.zeros_like(x), np.zeros_like(x)], -1)[None]
    m = np.float32(radius ** 2)
    query, cand = xyz(q[pick]), xyz(p[pick])
    brute = R.brute_knn(query, cand, 8, m)
    assert same(R.grid_knn(query, cand, 8, m, 0.0, R.default_cell(m)), brute)
    assert not same(R.grid_knn(query, cand, 8, m, 0.0, float(np.sqrt(np.float64(m)))), brute)


def scan_cloud(rng, n):
    """Scan-scale points in metres: a disc of 50 m around the sensor, denser near it, 4 m of height."""
    r = 50.0 * rng.random(n) ** 2 + 0.5
    a = 2 * np.pi * rng.random(n)
    return np.stack([r * np.cos(a), r * np.sin(a), 4 * rng.random(n) - 2], -1).astype(np.float32)[None]


@pytest.mark.parametrize("radius,K", [(0.5, 16), (1.0, 5), (3.0, 32)])
def test_grid_statement_equals_brute_force_on_scan_scale_clouds(radius, K):
    rng = np.random.default_rng(7)
    cand, query = scan_cloud(rng, 3000), scan_cloud(rng, 700)
    m = np.float32(radius ** 2)
    for origin in (0.0, (-3.25, 17.0, 0.125)):
        g = R.grid_knn(query, cand, K, m, origin, R.default_cell(m))
        assert same(g, R.brute_knn(query, cand, K, m)) and g["err_build"] == 0 and g["err_query"] == 0
    g = R.grid_knn(None, cand, K, m, 0.0, R.default_cell(m))
    assert same(g, R.brute_knn(None, cand, K, m))
    assert (g["idx"][0, :, 0] == np.arange(3000)).all() and (g["dist"][0, :, 0] == 0).all()        # every row finds itself first


def test_fma32_is_one_rounding_of_the_exact_sum():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    t = (rng.standard_normal(400) * 50).astype(np.float32)
    d = np.abs(rng.standard_normal(400) * 2500).astype(np.float32)
    got = R.fma32(t, d)
    for a, b, g in zip(t, d, got):
        exact = Fraction(float(a)) ** 2 + Fraction(float(b))
        near = np.float32(float(exact))
        best = min((np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))),
                   key=lambda x: abs(Fraction(float(x)) - exact))
        assert g == best


def test_lattice_cases_hold_ties_coincident_points_short_and_truncated_rows():
    """What the lattice cases of the GPU test are for, counted (the same generator, seed and shapes)."""
    rng = np.random.default_rng(11)
    N, M = 300, 1023
    cand, query = lattice(rng, 2, M), lattice(rng, 2, N)
    ties = coincident = short = truncated = 0
    for radius, K in ((0.25, 5), (0.5, 4), (1.0, 16), (2.0, 32)):
        m = np.float32(radius ** 2)
        g = R.grid_knn(query, cand, K + 1, m, 0.0, R.default_cell(m))
        ties += int((g["dist"][..., K - 1] == g["dist"][..., K]).sum() - np.isinf(g["dist"][..., K - 1]).sum())
        coincident += int((g["dist"][..., :2] == 0).all(-1).sum())
        short += int((g["count"] < K).sum())
        truncated += int((g["count"] > K).sum())
        assert same(g, R.brute_knn(query, cand, K + 1, m))
    assert ties > 200 and coincident > 20 and short > 100 and truncated > 200, (ties, coincident, short, truncated)


def _grid(origin=(0.0, 0.0, 0.0), cell=(1.0, 1.0, 1.0)):
    o, c = (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*cell)
    return o, c, ctypes.addressof(o), ctypes.addressof(c)


def test_refusals_need_no_gpu():
    lib = _lib.load()
    _o, _c, o, c = _grid()
    p = 4096                                   # a 16-byte aligned stand-in for a device pointer: nothing is launched, nothing dereferenced
    build = lambda cand=p, ld=3, B=1, M=8, og=o, ce=c, ws=p: lib.pn2_grid_build(cand, ld, B, M, None, og, ce, None, ws, None)
    knn = lambda q=p, ld=3, B=1, N=8, M=8, K=4, og=o, ce=c, ws=p, flags=0, idx=p: lib.pn2_grid_knn(q, ld, B, N, M, K, 1.0, None, og, ce, ws,
                                                                                                  flags, idx, None, None, None, None)
    for bad in (dict(cand=None), dict(og=None), dict(ce=None), dict(ws=None), dict(ld=2), dict(ld=17), dict(B=0), dict(B=65536), dict(M=0),
                dict(M=-1), dict(ws=p + 8)):
        assert build(**bad) == EINVAL, bad
    for bad in (dict(og=None), dict(ce=None), dict(ws=None), dict(idx=None), dict(ld=2), dict(ld=17), dict(B=0), dict(B=65536), dict(M=0),
                dict(N=0), dict(N=2 ** 31 - 255), dict(K=0), dict(K=-1), dict(ws=p + 8), dict(flags=2), dict(q=None, N=9)):
        assert knn(**bad) == EINVAL, bad
    assert knn(K=33) == EUNSUPPORTED and knn(K=1000) == EUNSUPPORTED
    for cell in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        _o2, _c2, o2, c2 = _grid(cell=cell)
        assert build(og=o2, ce=c2) == EINVAL and knn(og=o2, ce=c2) == EINVAL
    _o3, _c3, o3, c3 = _grid(origin=(0.0, float("inf"), 0.0))
    assert build(og=o3, ce=c3) == EINVAL and knn(og=o3, ce=c3) == EINVAL


def test_workspace_bytes_is_monotone_and_refuses_beyond_the_limits():
    lib = _lib.load()
    last = 0
    for M in (1, 2, 31, 32, 33, 64, 1000, 1023, 1024, 1025, 4096, 4097, 120000, 1 << 20, _lib.VOXEL_MAX_ROWS):
        n = lib.pn2_grid_workspace_bytes(1, M)
        assert n > last and n % 16 == 0 and n >= M * 16 + 2 * M * 16, M          # a record per row and a table of at least 2 M slots
        assert 2 * n < lib.pn2_grid_workspace_bytes(3, M) <= 3 * n        # (three clouds; the 16-byte rounding is shared)
        last = n
    for B, M in ((0, 8), (65536, 8), (1, 0), (1, -1), (1, _lib.VOXEL_MAX_ROWS + 1)):
        assert lib.pn2_grid_workspace_bytes(B, M) == EINVAL


def test_python_front_end_refuses_a_cell_below_the_radius():
    from pointnet12_amd import neighbors
    with pytest.raises(ValueError):
        neighbors.GridIndex(radius=1.0, cell=1.0)                     # below sqrt(max_d2) * (1 + 2^-20)
    with pytest.raises(ValueError):
        neighbors.GridIndex(max_d2=float("inf"))
    with pytest.raises(ValueError):
        neighbors.GridIndex()
    g = neighbors.GridIndex(radius=0.3)
    assert g.max_d2 == float(np.float32(0.3 ** 2)) and g.cell[0] == R.default_cell(np.float32(0.3 ** 2))
    assert neighbors.GridIndex(max_d2=float("inf"), cell=(1.0, 2.0, 3.0)).cell.tolist() == [1.0, 2.0, 3.0]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_grid_knn_kernels_do_not_spill():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "grid_knn.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
