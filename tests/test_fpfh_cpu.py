"""CPU: the numpy restatement of the FPFH rule (tests/fpfh_ref.py; include/pn2.h, "FPFH") held to cases worked by hand and to the
properties the rule promises -- exact invariance of the integer bins under motions that are exact in floating point, thirds that
sum to 200, the loop's weighted sum against a pairwise one -- and the binding table's two new entries."""
import os
import re

import numpy as np

import fpfh_ref as F
from conftest import ROOT
from pointnet12_amd import _lib


def _pair(ni, nj, pj=(1, 0, 0)):
    pts = np.array([[0, 0, 0], pj], np.float32)
    nrm = np.array([ni, nj], np.float32)
    idx = np.array([[1], [0]], np.int64)
    out, flagged, err = F.spfh_cloud(pts, nrm, idx)
    c, m = F.counts(out)
    return c, m, flagged, err


def test_pairs_worked_by_hand():
    # n_i = n_j = +z, dp = +x: a1 = a2 = 0, the frame stays on i; v = dp x n = -y, w = n x v = +x; f1 = atan2(0, 1) = 0, f2 = f3 = 0:
    # t = 5.5 three times
    c, m, flagged, err = _pair((0, 0, 1), (0, 0, 1))
    assert err == 0 and not flagged.any() and (m == 1).all()
    assert (np.nonzero(c[0])[0] == [5, 16, 27]).all() and (np.nonzero(c[1])[0] == [5, 16, 27]).all()
    # n_j = (0.6, 0, 0.8): a2 = 0.6 > a1 = 0, the frame moves to j: dp = -x, f3 = -0.6 -> t3 = 2.2; v = dp x n_s = (0, 0.8, 0) -> +y,
    # w = n_s x v = (-0.8, 0, 0.6); f2 = v . z = 0 -> 5.5; f1 = atan2(0.6, 0.8) = 0.6435 -> t1 = 11 (0.6435 + pi) / 2 pi = 6.63
    c, m, _, err = _pair((0, 0, 1), (0.6, 0, 0.8))
    assert err == 0 and (np.nonzero(c[0])[0] == [6, 16, 24]).all()
    # seen from j (row 1, dp = -x): a1 = (n_j . dp) = -0.6, a2 = (n_i . dp) = 0: the frame stays on j = this row's own point, same bins
    assert (c[1] == c[0]).all()
    # n_j = (0, 0.6, 0.8): a1 = a2 = 0; v = -y, f2 = v . n_j = -0.6 -> t2 = 2.2; f1 = atan2(w . n_j = 0, 0.8) = 0
    c, m, _, err = _pair((0, 0, 1), (0, 0.6, 0.8))
    assert (np.nonzero(c[0])[0] == [5, 13, 27]).all()
    # exactly antiparallel normals: n_s . n_t = -1, w . n_t = -0 + 0.0 = +0: f1 = +pi, t1 = 11, clamped to bin 10
    c, m, flagged, err = _pair((0, 0, 1), (0, 0, -1))
    assert c[0, 10] == 1 and c[0, :10].sum() == 0 and not flagged.any()
    # n_j along dp: the frame moves to j and v = dp x n_s = 0: not a pair; the rows are empty
    c, m, _, err = _pair((0, 0, 1), (1, 0, 0))
    assert (m == 0).all() and (c == 0).all() and err == F.ERR_EMPTY
    # a zero normal loses the pair silently, a NaN normal with a flag, a NaN point with a flag
    assert _pair((0, 0, 0), (0, 0, 1))[3] == F.ERR_EMPTY
    assert _pair((np.nan, 0, 0), (0, 0, 1))[3] == F.ERR_EMPTY | F.ERR_NONFINITE
    assert _pair((0, 0, 1), (0, 0, 1), pj=(np.inf, 0, 0))[3] == F.ERR_EMPTY | F.ERR_NONFINITE


def test_cut_off_duplicates_padding_and_repeats():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [3, 0, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    idx = np.array([[0, 2, 1, 1, 3, 4, -1]] * 4, np.int64)          # itself, a duplicate, a repeat, beyond the cut-off, padding, negative
    out, _, err = F.spfh_cloud(pts, nrm, idx, max_d2=4.0)
    c, m = F.counts(out)
    assert m.tolist() == [2, 3, 2, 2] and err == 0                  # row 3 reaches row 1 twice (d2 = 4 <= 4) and nothing else
    assert (out[:, 34:] == 0).all() and (c[:, :11].sum(1) == m).all() and (c[:, 11:22].sum(1) == m).all() and (c[:, 22:].sum(1) == m).all()
    out2, _, _ = F.spfh_cloud(pts, nrm, idx, max_d2=4.0, n=2)       # rows 2, 3 do not exist: row 0 keeps row 1 twice, row 1 keeps row 0
    assert out2.shape == (2, 36) and F.counts(out2)[1].tolist() == [2, 1]


def test_plane_lattice_uses_one_bin_per_third():
    pts, nrm = F.plane_lattice()
    idx = F.knn_self(pts, 9)
    out, flagged, err = F.spfh_cloud(pts, nrm, idx)
    c, m = F.counts(out)
    assert err == 0 and not flagged.any() and (m == 8).all()
    assert (c[:, [5, 16, 27]] == 8).all() and c.sum() == 3 * 8 * 64
    f, _, voters, _ = F.finish_cloud(pts, idx, out)
    assert (voters == 8).all() and np.abs(f[:, [5, 16, 27]] - 200.0).max() <= 1e-9 and abs(f.sum() - 600.0 * 64) <= 1e-6


def test_bins_are_exactly_invariant_under_exact_motions():
    pts, nrm = F.wavy_sheet()
    idx = F.knn_self(pts, 16)
    base, flagged, err = F.spfh_cloud(pts, nrm, idx, edge=1e-6)
    assert err == 0 and not flagged.any() and (F.counts(base)[1] == 15).all()
    cyc, _, _ = F.spfh_cloud(pts[:, [1, 2, 0]].copy(), nrm[:, [1, 2, 0]].copy(), idx)          # (x, y, z) -> (y, z, x)
    assert (cyc == base).all()
    half = np.array([-1, -1, 1], np.float32)                                                 # the half-turn about z
    rot, _, _ = F.spfh_cloud(pts * half, nrm * half, idx)
    assert (rot == base).all()
    lp, ln = F.lattice()
    _, flagged, err = F.spfh_cloud(lp, ln, F.knn_self(lp, 16), edge=1e-6)
    assert err == 0 and not flagged.any()


def test_thirds_sum_to_200_and_the_loop_matches_a_pairwise_sum():
    for (pts, nrm), k, max_d2 in ((F.wavy_sheet(), 16, np.inf), (F.lattice(), 32, 0.3), (F.wavy_sheet(), 8, 0.05)):
        idx = F.knn_self(pts, k)
        out, _, _ = F.spfh_cloud(pts, nrm, idx, max_d2)
        f32, f, voters, _ = F.finish_cloud(pts, idx, out, max_d2)
        live = (F.counts(out)[1] > 0) & (voters > 0)
        assert live.sum() > len(pts) // 2
        for third in range(3):
            assert np.abs(f[live, 11 * third:11 * third + 11].sum(1) - 200.0).max() <= 1e-9
        g = F.finish_cloud(pts, idx, out, max_d2, reduce=True)[1]
        assert (np.abs(f - g) <= 2.0 ** -45 * np.abs(g)).all()
        assert (f32 == f.astype(np.float32)).all()


def test_header_table_and_constants_agree():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+15\b", text) and _lib.ABI_VERSION == 15
    assert re.search(r"#define\s+PN2_FPFH_ERR_EMPTY\s+%d\b" % _lib.FPFH_ERR_EMPTY, text)
    assert re.search(r"#define\s+PN2_FPFH_ERR_NONFINITE\s+%d\b" % _lib.FPFH_ERR_NONFINITE, text)
    assert (F.ERR_EMPTY, F.ERR_NONFINITE) == (_lib.FPFH_ERR_EMPTY, _lib.FPFH_ERR_NONFINITE)
    assert len(_lib.SIGNATURES["pn2_spfh"][1]) == 14 and len(_lib.SIGNATURES["pn2_fpfh"][1]) == 12
    assert os.path.exists(os.path.join(_lib.CSRC, "fpfh.hip"))
