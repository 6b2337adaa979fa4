"""CPU: the segmentation-metrics contract that needs no device.  The C entry point (pn2_seg_confusion, added within ABI 15) is
declared, bound and exported and its argument checks are host code; tests/metrics_ref.py -- the yardstick of
tests/test_metrics_gpu.py -- reproduces BIT FOR BIT what the reference's own pcd_utils.py returned for the recorded cases
(tests/golden/g16_metrics.npz, tools/make_golden_metrics.py) when it is fed the integer tables alone; the public names carry the
reference's parameter names."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import metrics_ref as R

from pointnet12_amd import _lib

CASES = ("s13", "k20", "p50", "ties", "special", "c1", "clf")


def G():
    return golden("g16_metrics.npz")


def batch_tables(g, c, per_cloud):
    """The recorded per-cloud tables of case c cut into its batches; pooled per batch unless per_cloud."""
    parts = np.split(g[c + "/tables"], int(g[c + "/nbatch"]))
    return parts if per_cloud else [p.sum(0) for p in parts]


def batch_points(g, c):
    B, N = g[c + "/target"].shape
    return [B // int(g[c + "/nbatch"]) * N] * int(g[c + "/nbatch"])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_entry_point_is_declared_bound_and_exported_within_abi_15():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+15\b", text) and _lib.ABI_VERSION == 15
    assert re.search(r"\bint\s+pn2_seg_confusion\s*\(", text) and "added within ABI 15" in text
    res, args = _lib.SIGNATURES["pn2_seg_confusion"]
    assert res is ctypes.c_int and len(args) == 11
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pn2_seg_confusion")
    assert _lib.load().pn2_version() == 15


def test_argument_checks_are_host_code():
    lib = _lib.load()
    one = ctypes.c_void_p(256)                                 # a non-NULL placeholder: refused shapes launch nothing
    none = -2 ** 63
    assert lib.pn2_seg_confusion(None, 16, one, 1, 8, 13, none, one, 0, None, None) == -1
    assert lib.pn2_seg_confusion(one, 16, None, 1, 8, 13, none, one, 0, None, None) == -1
    assert lib.pn2_seg_confusion(one, 16, one, 1, 8, 13, none, None, 0, None, None) == -1
    assert lib.pn2_seg_confusion(one, 0, one, 1, 8, 13, none, one, 0, None, None) == -1
    assert lib.pn2_seg_confusion(one, 16, one, -1, 8, 13, none, one, 0, None, None) == -1
    assert lib.pn2_seg_confusion(one, 16, one, 1, -8, 13, none, one, 0, None, None) == -1
    assert lib.pn2_seg_confusion(one, 16, one, 1, 8, 0, none, one, 0, None, None) == -1
    assert lib.pn2_seg_confusion(one, 12, one, 1, 8, 13, none, one, 0, None, None) == -1          # pitch below C
    assert lib.pn2_seg_confusion(one, 16, one, 1, 8, 13, none, one, 13, None, None) == -1         # tables would overlap
    assert lib.pn2_seg_confusion(one, 16, one, 1, 8, 13, none, one, -1, None, None) == -1
    assert lib.pn2_seg_confusion(one, 68, one, 1, 8, 65, none, one, 0, one, None) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_seg_confusion(one, 16, one, 1, 0, 13, none, one, 0, one, None) == 0
    assert lib.pn2_seg_confusion(one, 16, one, 0, 8, 13, none, one, 14 * 13, None, None) == 0


def test_restatement_reproduces_the_reference_bit_for_bit():
    g = G()
    assert tuple(str(c) for c in g["cases"]) == CASES
    empty = 0
    for c in CASES:
        C = g[c + "/logp"].shape[-1]
        assert g[c + "/logp"].dtype == np.float32 and g[c + "/tables"].dtype == np.int64
        calc = np.zeros((C, 3))
        for t in batch_tables(g, c, False):
            calc = R.calc_categorical_iou(t, C, calc)
        assert np.array_equal(bits(calc[:, :2]), bits(g[c + "/calc_tabel"])), c
        cat, lst = np.zeros((C, 3)), []
        for ts in batch_tables(g, c, True):
            cat, more = R.compute_cat_iou(ts, C, cat)
            lst += more
        assert np.array_equal(bits(cat[:, :2]), bits(g[c + "/cat_tabel"])), c
        assert np.array_equal(bits(lst), bits(g[c + "/cat_list"])), c
        assert len(lst) == g[c + "/tables"].shape[0] * C
        empty += sum(1 for v in lst if type(v) is int)
    assert empty > 100                                           # U == 0 -> the integer 1, many times (p50)


def test_golden_predictions_and_tables_are_what_plain_counting_gives():
    g = G()
    for c in CASES:
        logp, target, pred = g[c + "/logp"], g[c + "/target"], g[c + "/pred"]
        C = logp.shape[-1]
        assert np.array_equal(pred, R.argmax_lowest(logp)), c
        slow = np.zeros_like(g[c + "/tables"])
        for b in range(pred.shape[0]):
            for n in range(pred.shape[1]):
                t = int(target[b, n])
                slow[b, t if 0 <= t < C else C, pred[b, n]] += 1
        assert np.array_equal(slow, g[c + "/tables"]), c
        assert np.array_equal(R.count_tables(pred, target, C), slow), c
        assert slow.sum() == target.size
    assert np.array_equal(g["ties/pred"], g["ties/expected"]) and g["ties/pred"].shape[1] >= 100
    shared = (g["ties/logp"] == g["ties/logp"].max(-1, keepdims=True)).sum(-1)
    assert set(np.unique(shared)) == {2, 3}
    sp = g["special/logp"]
    assert np.isnan(sp).any(-1).sum() >= 4 and np.isneginf(sp).all(-1).sum() >= 2
    assert {-1, 13, 255} <= set(g["special/target"].reshape(-1).tolist()) and g["special/tables"][:, 13].sum() >= 10
    assert g["c1/logp"].shape[-1] == 1 and g["p50/logp"].shape == (4, 512, 50)
    I, U = R.iou_counts(g["p50/tables"][0])
    assert (U == 0).sum() > 40                                    # a shape holds the parts of ONE category


def test_restated_loops_reproduce_the_reference_loops():
    """test_semseg / test_partseg / test_clf of pcd_utils.py were run unmodified on the recorded batches: the restatement over
    integer tables gives their numbers -- exactly where the reference adds plainly, within 4 ulp where pandas sums a group."""
    g = G()
    acc, iou, cat_iou, _ = R.test_semseg(batch_tables(g, "s13", False), batch_points(g, "s13"), list(g["s3dis_names"]), 13)
    assert bits(acc) == bits(g["loop_semseg/accuracy"]) and bits(iou) == bits(g["loop_semseg/iou"])
    assert list(cat_iou) == [str(n) for n in g["loop_semseg/names"]] == sorted(cat_iou)
    assert max(R.ulps(a, b) for a, b in zip(cat_iou.values(), g["loop_semseg/cat_iou"])) <= 4

    metrics, hist, cat_iou = R.test_partseg(batch_tables(g, "p50", True), batch_points(g, "p50"), list(g["part_names"]), 50)
    assert bits(metrics["accuracy"]) == bits(g["loop_partseg/accuracy"])
    assert bits(metrics["inctance_avg_iou"]) == bits(g["loop_partseg/inctance_avg_iou"])
    assert np.array_equal(bits(hist), bits(g["loop_partseg/hist_acc"]))
    assert list(cat_iou) == [str(n) for n in g["loop_partseg/names"]] and len(cat_iou) == 16
    assert max(R.ulps(a, b) for a, b in zip(cat_iou.values(), g["loop_partseg/cat_iou"])) <= 4
    assert R.ulps(metrics["class_avg_iou"], g["loop_partseg/class_avg_iou"]) <= 4

    assert bits(R.test_clf(batch_tables(g, "clf", False), [8, 8, 8])) == bits(g["loop_clf/accuracy"])

    acc, miou, per_class = R.test_kitti_semseg(batch_tables(g, "k20", False), batch_points(g, "k20"), 20)
    assert per_class.dtype == np.float64 and 0 < miou < 1 and 0 < acc < 1
    I, U = R.iou_counts(g["k20/tables"].sum(0))
    assert I.sum() == acc * g["k20/target"].size                  # (equal batch sizes: the mean of quotients is the pooled one)


def test_cpu_tensors_and_other_dtypes_are_refused():
    from pointnet12_amd import metrics as M
    with pytest.raises(_lib.Pn2Error):
        M.confusion(torch.zeros(2, 8, 13), torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(_lib.Pn2Error):
        M.calc_categorical_iou(torch.zeros(2, 8, 13), torch.zeros(2, 8, dtype=torch.int64), 13, np.zeros((13, 3)))
    with pytest.raises(_lib.Pn2Error):
        M.compute_cat_iou(torch.zeros(2, 8, 13), torch.zeros(2, 8, dtype=torch.int64), 13, np.zeros((13, 3)))
    with pytest.raises(_lib.Pn2Error):
        M.SegEvaluator(13).update(torch.zeros(2, 8, 13), torch.zeros(2, 8, dtype=torch.int64))


def test_public_names_carry_the_reference_parameter_names():
    from pointnet12_amd import metrics as M
    want = {
        "to_categorical": ["y", "num_classes"],
        "calc_categorical_iou": ["pred", "target", "num_classes", "iou_tabel"],
        "compute_cat_iou": ["pred", "target", "num_classes", "iou_tabel"],
        "test_clf": ["model", "loader"],
        "test_partseg": ["model", "loader", "catdict", "model_name", "num_classes"],
        "test_semseg": ["model", "loader", "catdict", "model_name", "num_classes"],
        "test_kitti_semseg": ["model", "loader", "model_name", "num_classes", "class_names"],
        "confusion": ["log_probs", "target", "num_classes", "per_cloud", "out", "ignore_index", "return_pred"],
        "iou_counts": ["conf"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(M, name)).parameters) == params, name
    assert inspect.signature(M.test_partseg).parameters["num_classes"].default == 50
    assert list(inspect.signature(M.SegEvaluator.__init__).parameters) == ["self", "num_classes", "per_cloud"]
    assert not hasattr(M, "compute_overall_iou")
    # to_categorical and iou_counts need no device
    assert M.to_categorical(torch.tensor([[0, 2], [1, 1]]), 3).tolist() == [[[1, 0, 0], [0, 0, 1]], [[0, 1, 0], [0, 1, 0]]]
    assert M.to_categorical(torch.tensor([1]), 4).dtype == torch.float32
    g = G()
    for conf in (g["special/tables"], torch.from_numpy(g["special/tables"])):
        I, U = M.iou_counts(conf)
        for b in range(2):
            ri, ru = R.iou_counts(g["special/tables"][b])
            assert np.array_equal(np.asarray(I[b]), ri) and np.array_equal(np.asarray(U[b]), ru)
