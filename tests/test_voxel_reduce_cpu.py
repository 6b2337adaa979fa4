"""CPU: the segment-reduction rules (include/pn2.h, ``pn2_segment_mean`` / ``pn2_segment_mode``) as tests/voxel_reduce_ref.py states
them -- the mean against the exact mean (``fractions.Fraction``) within the DERIVED bound and bit-identical under permutation, the
mode against ``collections.Counter`` -- and the entry points' argument checks (no launch, no GPU) and "no scratch" for
csrc/voxel_reduce.hip."""
import collections
import ctypes
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import voxel_reduce_ref as R
from conftest import ROOT
from pointnet12_amd import _lib

F32_MAX = np.finfo(np.float32).max
TINY = np.float32(2.0 ** -149)


def columns(rng):
    """Named float32 columns of finite terms, each one segment."""
    out = {}
    for n in (1, 2, 3, 17, 400):
        out["normal%d" % n] = rng.normal(scale=3.0, size=n)
        out["decades%d" % n] = rng.normal(size=n) * 10.0 ** rng.uniform(-38, 38, size=n)       # spreads far beyond 34 bits
        out["subnormal%d" % n] = rng.integers(-(1 << 23) + 1, 1 << 23, size=n) * 2.0 ** -149
        out["around_min_normal%d" % n] = rng.uniform(-4.0, 4.0, size=n) * 2.0 ** -126
    out["spread_just_inside"] = [1.0, 2.0 ** -33, -(2.0 ** -33), 2.0 ** -32]                       # K - k = 33: one bit survives
    out["spread_just_outside"] = [1.0, 2.0 ** -34, 2.0 ** -34, 2.0 ** -40]                         # K - k >= 34: the terms vanish
    out["truncated_negatives"] = [4.0] + [-(1.0 + 2.0 ** -23) * 2.0 ** -20] * 50                   # magnitudes truncate: toward zero
    out["cancel"] = [3.25, -3.25]
    out["cancel_many"] = np.concatenate([np.arange(1, 60) * 0.37, -np.arange(1, 60) * 0.37])
    out["cancel_large_leaves_small"] = [1e30, -1e30, 1.5]
    out["overflowing_sum"] = [3e38, 3e38, 3e38]
    out["overflowing_sum_max"] = [F32_MAX] * 200
    out["overflowing_negative"] = [-F32_MAX, -F32_MAX, -3e38]
    out["max_and_tiny"] = [F32_MAX, TINY, -TINY]
    out["zeros"] = [0.0, -0.0, 0.0]
    out["negative_zeros"] = [-0.0, -0.0]
    out["one_subnormal"] = [TINY]
    out["subnormal_mean_of_normals"] = [2.0 ** -126, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]                 # the MEAN is subnormal
    return {k: np.asarray(v, np.float64).astype(np.float32) for k, v in out.items()}


def test_restatement_against_the_exact_mean_within_the_derived_bound():
    cols = columns(np.random.default_rng(0))
    worst = Fraction(0)
    for name, col in cols.items():
        assert np.isfinite(col).all(), name
        ref = R.segment_mean(col[:, None], np.zeros(len(col), np.int32), 1)
        mean, K = ref["mean"][0, 0], ref["K"][0, 0]
        assert ref["err"] == 0 and ref["n"][0] == len(col) and np.isfinite(mean), name
        exact = R.exact_mean(col)
        bound = R.mean_bound(K, exact, mean)
        miss = abs(Fraction(float(mean)) - exact)
        assert miss <= bound, (name, float(miss), float(bound))
        worst = max(worst, miss / bound)
    assert worst > Fraction(1, 4)                                     # (the cases do come near the bound: it is not slack by orders)
    # planted values
    one = lambda v: R.segment_mean(np.asarray(v, np.float32)[:, None], np.zeros(len(v), np.int32), 1)["mean"].view(np.uint32)[0, 0]
    assert one(cols["cancel"]) == 0 and one(cols["cancel_many"]) == 0 and one(cols["zeros"]) == 0 and one(cols["negative_zeros"]) == 0
    assert one(cols["overflowing_sum"]) == np.float32(3e38).view(np.uint32)
    assert one(cols["overflowing_sum_max"]) == np.float32(F32_MAX).view(np.uint32)
    assert one(cols["one_subnormal"]) == 1 and one([1.0, 2.0 ** -34, 2.0 ** -34]) == np.float32(1.0 / 3.0).view(np.uint32)
    assert one(cols["cancel_large_leaves_small"]) == 0                # 1.5 lies more than 34 bits below 1e30: it vanishes, within the bound
    assert one([5.0]) == np.float32(5.0).view(np.uint32) and one([-7.5, -7.5]) == np.float32(-7.5).view(np.uint32)


def test_restatement_is_bit_identical_under_row_permutation():
    rng = np.random.default_rng(1)
    M, C, count = 3000, 5, 40
    values = (rng.normal(size=(M, C)) * 10.0 ** rng.uniform(-30, 30, size=(M, C))).astype(np.float32)
    values[:200, 1] = (rng.integers(-1000, 1000, 200) * 2.0 ** -149).astype(np.float32)
    seg = rng.integers(-1, count, M).astype(np.int32)                 # some rows take no part
    ref = R.segment_mean(values, seg, count)
    assert ref["err"] == 0 and ref["n"].sum() == (seg >= 0).sum()
    for seed in range(4):
        perm = np.random.default_rng(seed + 10).permutation(M)
        again = R.segment_mean(values[perm], seg[perm], count)
        assert np.array_equal(again["mean"].view(np.uint32), ref["mean"].view(np.uint32)) and np.array_equal(again["n"], ref["n"])
        assert np.array_equal(again["S"], ref["S"]) and np.array_equal(again["K"], ref["K"])
    # an empty segment gives +0.0; a NaN / inf poisons its own column of its own segment only and sets the bit
    assert (R.segment_mean(values, np.where(seg == 3, -1, seg), count)["mean"].view(np.uint32)[3] == 0).all()
    bad = values.copy()
    rows7 = np.flatnonzero(seg == 7)
    bad[rows7[0], 2], bad[rows7[1], 4], bad[rows7[2], 4] = np.nan, np.inf, np.inf
    got = R.segment_mean(bad, seg, count)
    assert got["err"] == R.ERR_NONFINITE
    expect = ref["mean"].view(np.uint32).copy()
    expect[7, 2] = expect[7, 4] = R.QUIET_NAN                         # (infinities of one sign too: the stated deviation)
    assert np.array_equal(got["mean"].view(np.uint32), expect)
    # a segment at or beyond the count takes no part and sets its bit
    far = seg.copy()
    far[5] = count
    got = R.segment_mean(values, far, count)
    assert got["err"] == R.ERR_RANGE and np.array_equal(got["mean"].view(np.uint32), R.segment_mean(values, np.where(far == count, -1, far), count)["mean"].view(np.uint32))


def test_backward_restatement():
    g = np.arange(12, dtype=np.float32).reshape(4, 3) / np.float32(7.0)
    seg = np.array([0, 3, -1, 3, 3, 1, 9], np.int32)
    n = np.array([1, 1, 0, 3], np.int32)
    got, err = R.segment_mean_bwd(g, seg, 4, n)
    assert err == R.ERR_RANGE and got.dtype == np.float32
    assert np.array_equal(got[1], g[3] / np.float32(3.0)) and np.array_equal(got[0], g[0]) and not got[2].any() and not got[6].any()
    assert not np.signbit(got[2]).any()


def test_mode_restatement_against_counter_with_ties():
    rng = np.random.default_rng(2)
    M, count = 4000, 300
    labels = rng.integers(-2, 6, M).astype(np.int32)                  # few classes over many rows: ties are certain
    labels[rng.integers(0, M, 40)] = 2 ** 31 - 1
    seg = rng.integers(-1, count + 1, M).astype(np.int32)
    seg[seg == count] = count - 1
    seg[(seg == 11) | (seg == 12)] = 13                               # segments 11 and 12: empty
    labels[seg == 20] = -1                                            # segment 20: negative labels only
    winner, votes, err = R.segment_mode(labels, seg, count, fill=-5)
    ties = 0
    for s in range(count):
        c = collections.Counter(int(l) for l in labels[seg == s] if l >= 0)
        if not c:
            assert winner[s] == -5 and votes[s] == 0
            continue
        best = max(c.values())
        tied = sorted(l for l, v in c.items() if v == best)
        ties += len(tied) > 1
        assert winner[s] == tied[0] and votes[s] == best, s
    assert err == 0 and ties > 20 and winner[11] == winner[12] == winner[20] == -5
    w, v, err = R.segment_mode([3, 3, 1, 1, 0], [0, 0, 0, 0, 5], 2)
    assert err == R.ERR_RANGE and w.tolist() == [1, -1] and v.tolist() == [2, 0]


def test_error_bits_match_the_header():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for name, value in (("PN2_SEGMENT_ERR_RANGE", _lib.SEGMENT_ERR_RANGE), ("PN2_SEGMENT_ERR_NONFINITE", _lib.SEGMENT_ERR_NONFINITE),
                        ("PN2_SEGMENT_MAX_COLS", _lib.SEGMENT_MAX_COLS)):
        assert "#define %s %d\n" % (name, value) in text
    assert (R.ERR_RANGE, R.ERR_NONFINITE) == (_lib.SEGMENT_ERR_RANGE, _lib.SEGMENT_ERR_NONFINITE)
    bits = [_lib.VOXEL_ERR_RANGE, _lib.VOXEL_ERR_ROWS, _lib.SEGMENT_ERR_RANGE, _lib.SEGMENT_ERR_NONFINITE]
    assert sorted(bits) == [1, 2, 4, 8]                               # one error word serves the grid and its reductions


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    a = 4096                                                          # a non-null, aligned stand-in: a refused call touches nothing
    vp = lambda x: ctypes.c_void_p(x)
    EINVAL = -1

    def mean(values=a, ld=4, C=4, seg=a, begin=a, count=a, B=1, max_rows=16, out_begin=a, out_count=a, out=a, ld_out=4, workspace=a):
        return lib.pn2_segment_mean(vp(values), ld, C, vp(seg), vp(begin), vp(count), B, max_rows, vp(out_begin), vp(out_count), None,
                                    vp(out), ld_out, None, None, vp(workspace), None)

    def bwd(grad_out=a, ld_out=4, C=4, seg=a, begin=a, count=a, B=1, max_rows=16, out_begin=a, out_count=a, n=a, grad_in=a, ld_in=4):
        return lib.pn2_segment_mean_bwd(vp(grad_out), ld_out, C, vp(seg), vp(begin), vp(count), B, max_rows, vp(out_begin), vp(out_count),
                                        vp(n), vp(grad_in), ld_in, None, None)

    def mode(labels=a, seg=a, begin=a, count=a, B=1, max_rows=16, out_begin=a, out_count=a, out=a, votes=None, workspace=a):
        return lib.pn2_segment_mode(vp(labels), vp(seg), vp(begin), vp(count), B, max_rows, vp(out_begin), vp(out_count), -1, vp(out),
                                    vp(votes), None, vp(workspace), None)

    for name in ("values", "seg", "begin", "count", "out_begin", "out_count", "out", "workspace"):
        assert mean(**{name: None}) == EINVAL, name
    for name in ("grad_out", "seg", "begin", "count", "out_begin", "out_count", "n", "grad_in"):
        assert bwd(**{name: None}) == EINVAL, name
    for name in ("labels", "seg", "begin", "count", "out_begin", "out_count", "workspace"):
        assert mode(**{name: None}) == EINVAL, name
    assert mode(out=None, votes=None) == EINVAL                       # nothing to write
    for call in (mean, bwd):
        assert call(C=0) == EINVAL and call(C=17) == EINVAL and call(C=-1) == EINVAL
        assert call(ld_out=3) == EINVAL                               # a pitch below C
    assert mean(ld=3) == EINVAL and bwd(ld_in=3) == EINVAL and mean(ld=16, C=16, ld_out=15) == EINVAL
    for call in (mean, bwd, mode):
        assert call(B=0) == EINVAL and call(B=-3) == EINVAL and call(B=65536) == EINVAL
        assert call(max_rows=-1) == EINVAL and call(max_rows=_lib.VOXEL_MAX_ROWS + 1) == EINVAL
    assert mean(values=a + 2) == EINVAL and mean(workspace=a + 8) == EINVAL and mode(workspace=a + 8) == EINVAL and mode(labels=a + 1) == EINVAL
    wb = lib.pn2_segment_reduce_workspace_bytes
    assert wb(0, 16, 4) == EINVAL and wb(1, -1, 4) == EINVAL and wb(65536, 16, 4) == EINVAL and wb(1, _lib.VOXEL_MAX_ROWS + 1, 4) == EINVAL
    assert wb(1, 16, 0) == EINVAL and wb(1, 16, 17) == EINVAL and wb(1, 0, 1) > 0 and wb(1, 1 << 22, 16) > 0
    for C in (1, 4, 16):
        sizes = [wb(1, m, C) for m in (0, 1, 63, 1024, 1025, 4096, 120000, 131071, 1 << 22)]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)              # monotone in max_rows
        by_b = [wb(B, 5000, C) for B in (1, 2, 3, 16, 65535)]
        assert all(s > 0 and s % 16 == 0 for s in by_b) and by_b == sorted(set(by_b))            # ... and strictly in B
        for m in (1, 1000, 120000):                                   # enough for either: the mean's accumulators, the mode's table
            assert wb(1, m, C) >= max(12 * m * C + 4 * m, 2 * m * 16 + 8 * m)
    assert [wb(1, 120000, C) for C in (1, 4, 16)] == sorted(wb(1, 120000, C) for C in (1, 4, 16))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_reduce_kernels_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "voxel_reduce.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
