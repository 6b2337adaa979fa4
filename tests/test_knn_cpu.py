"""CPU: what of the k-nearest-neighbour family (csrc/knn.hip, pointnet_util.knn_point / propagate_labels, kitti.write_labels)
needs no device -- that the lattice cases of tests/test_knn_gpu.py exercise the tie rules they are there for, the fp64
statements themselves on rows worked out by hand, the ``.label`` writer, the argument checks of the two entry points, and
that no instantiation of the kernels spills."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import knn_ref as KR

from pointnet12_amd import _lib, kitti
from pointnet12_amd import pointnet_util as U


def test_lattice_cases_hold_what_they_are_for():
    """Ties across the cut in at least 40 % of the queries for every K, coincident points, tied votes in at least 40 % of
    the rows for K >= 5, and between 30 % and 70 % of the rows without a voter at cut-off 0."""
    for N, M in KR.LATTICE_CASES[1:]:
        order, ds = KR.lattice_sorted(N, M)
        ties = [(ds[..., K - 1] == ds[..., K]).mean() for K in range(1, 33)]
        print("(N, M) = (%d, %d): ties at the cut %.2f .. %.2f" % (N, M, min(ties), max(ties)))
        assert min(ties) >= 0.40, (N, M, ties)
        assert (ds[..., 0] == 0).any()
    N, M = KR.LATTICE_CASES[0]                             # M = 33: K = 32 = M - 1 leaves one candidate out
    order, ds = KR.lattice_sorted(N, M)
    assert (ds[..., 31] == ds[..., 32]).any()
    N, M = KR.VOTE_CASE
    q, c, labels = KR.lattice_case(N, M)
    order, ds = KR.lattice_sorted(N, M)
    for K in KR.VOTE_KS[1:]:
        tied = np.mean([KR.has_tied_vote(order[b, n, :K], ds[b, n, :K], labels[b], M, np.inf) for b in range(KR.B) for n in range(N)])
        print("K = %d: tied votes %.2f" % (K, tied))
        assert tied >= 0.40, (K, tied)
    none = (ds[..., 0] > 0).mean()
    print("rows with no voter at cut-off 0: %.2f" % none)
    assert 0.30 <= none <= 0.70
    idx, dist = KR.knn64(q, c, 17)                         # the prefix of the full sort IS knn64
    assert (idx == order[..., :17]).all() and (dist == ds[..., :17]).all()


def test_the_statements_on_rows_worked_out_by_hand():
    c = np.float32([[[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 0]]])
    q = np.float32([[[0, 0, 0], [1, 0, 0]]])
    idx, dist = KR.knn64(q, c, 4)
    assert idx.tolist() == [[[0, 4, 1, 2], [1, 2, 0, 4]]] and dist.tolist() == [[[0, 0, 1, 1], [0, 0, 1, 1]]]
    labels = np.int64([[7, 9, 9, 3, 5]])
    # row 0: 7, 5, 9, 9 -> 9 has two votes; with cut-off 0 only 7 and 5 vote, one each: the nearer first slot (7) wins
    assert KR.vote_row(idx[0, 0], dist[0, 0], labels[0], 5, np.inf) == (9, 4)
    assert KR.vote_row(idx[0, 0], dist[0, 0], labels[0], 5, 0.0) == (7, 2)
    assert KR.vote_row(np.int64([5, -1]), np.float64([0, 0]), labels[0], 5, np.inf) == (None, 0)       # sentinels do not vote
    assert KR.has_tied_vote(idx[0, 0], dist[0, 0], labels[0], 5, 0.0) and not KR.has_tied_vote(idx[0, 0], dist[0, 0], labels[0], 5, np.inf)
    lut = np.int32([10, 11, 12, 13, 14, 15, 16, 17])      # label 9 is outside: fill and err bit 1
    out, err = KR.vote_ref(idx, dist, labels, 5, np.inf, -1, lut=lut)
    assert out.tolist() == [[-1, -1]] and err == 1
    out, err = KR.vote_ref(idx, dist, labels, 5, 0.0, -1, lut=lut, dst=np.int32([[2, 3]]), out=np.full((1, 3), 99, np.int32))
    assert out.tolist() == [[99, 99, 17]] and err == 3     # row 1: 9 and 9 at d = 0, outside the lut, AND its dst is out of range
    out, err = KR.vote_ref(idx, dist, labels, 5, np.inf, -1, n_query=[1])
    assert out.tolist() == [[9, -1]] and err == 0


def test_label_file_round_trip(tmp_path):
    g = golden("g18_kitti_view.npz")
    inv = dict(zip(g["learning_map_inv_keys"].tolist(), g["learning_map_inv_values"].tolist()))
    lut = kitti.inverse_label_lut(inv, device="cpu")
    K = max(inv)
    assert lut.dtype == torch.int32 and lut.shape == (K,) and lut.tolist() == [inv[c + 1] for c in range(K)]
    rng = np.random.default_rng(0)
    pred = rng.integers(0, K, 1000)
    ids = lut.numpy()[pred]
    ids[::7] = 0                                          # rows without a label
    fn = str(tmp_path / "000000.label")
    kitti.write_labels(fn, torch.from_numpy(ids))
    assert os.path.getsize(fn) == 4 * len(ids)
    words = np.fromfile(fn, np.uint32)
    assert ((words & 0xFFFF) == ids).all() and ((words >> 16) == 0).all()
    assert np.frombuffer(open(fn, "rb").read(), "<u4").tolist() == ids.tolist()           # little-endian words
    kitti.write_labels(fn, ids.astype(np.int64))
    assert (np.fromfile(fn, np.uint32) == ids).all()
    for bad in (np.int32([0, -1]), np.int64([70000]), np.float32([1.0])):
        with pytest.raises(ValueError):
            kitti.write_labels(fn, bad)
    with pytest.raises(ValueError):
        kitti.inverse_label_lut({0: 0, 2: 10}, device="cpu")


def test_entry_points_and_their_refusals_need_no_gpu():
    lib = _lib.load()
    assert len(_lib.SIGNATURES["pn2_knn"][1]) == 11 and len(_lib.SIGNATURES["pn2_knn_vote"][1]) == 17
    p = 4096                                              # (never dereferenced: every call below returns before a launch)
    assert lib.pn2_knn(p, p, 1, 8, 40, 33, None, None, p, None, None) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_knn(p, p, 1, 8, 8, 9, None, None, p, None, None) == -1                  # K > M
    assert lib.pn2_knn(p, p, 1, 8, 8, 0, None, None, p, None, None) == -1
    assert lib.pn2_knn(None, p, 1, 8, 8, 3, None, None, p, None, None) == -1
    assert lib.pn2_knn(p, p, 1, 0, 8, 3, None, None, p, None, None) == -1
    assert lib.pn2_knn_vote(p, p, p, 1, 8, 8, 33, 1.0, None, 0, None, 0, None, 8, p, None, None) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_knn_vote(p, p, p, 1, 8, 8, 0, 1.0, None, 0, None, 0, None, 8, p, None, None) == -1
    assert lib.pn2_knn_vote(p, p, p, 1, 8, 8, 3, 1.0, None, 0, None, 0, None, 7, p, None, None) == -1      # out_stride < N, no dst
    assert lib.pn2_knn_vote(p, None, p, 1, 8, 8, 3, 1.0, None, 0, None, 0, None, 8, p, None, None) == -1
    with pytest.raises(_lib.Pn2Error):
        U.knn_point(3, torch.zeros(1, 8, 3), torch.zeros(1, 2, 3))
    with pytest.raises(_lib.Pn2Error):
        U.propagate_labels(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int64))


def test_set_abstraction_keeps_its_state_dict_with_knn():
    a = U.PointNetSetAbstraction(16, 0.2, 8, 6, [16, 32], False)
    b = U.PointNetSetAbstraction(16, 0.2, 8, 6, [16, 32], False, knn=True)
    assert list(a.state_dict()) == list(b.state_dict()) and b.knn and not a.knn
    b.load_state_dict(a.state_dict())


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_no_instantiation_of_the_knn_kernels_spills():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "knn.hip"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
