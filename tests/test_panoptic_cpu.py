"""CPU: the panoptic-quality rule of include/pn2.h as tests/panoptic_ref.py states it -- the integer threshold and the integrality of
``q * 2^53`` it rests on, the stated deviation from the API's running fp64 sum, hand-worked tables written out as literals (the
reference is not only tested against itself), mutants of the rule, and ``kitti.split_label_words``."""
import numpy as np
import pytest
import torch

import panoptic_ref as R
from pointnet12_amd import _lib, kitti

CALL = ("include", "things", "min_points", "begins", "counts")


def table_of(case, **kw):
    return R.panoptic_table(case["pred_sem"], case["pred_inst"], case["gt_sem"], case["gt_inst"], case["C"],
                            **{k: case[k] for k in CALL}, **kw)


def generated():
    """The seeded cases the deviation bound is held on: one and several clouds, few and many segments."""
    for seed in range(12):
        yield R.random_case(seed, 400 + 37 * seed, C=3 + seed % 4, segments=4 + 3 * seed, B=1 + seed % 3)
    yield R.random_case(100, 60000, C=6, segments=1500, B=1, noise=0.01, ids=1 << 20)


def test_integer_threshold_equals_the_fp64_quotient_and_the_scaled_quotient_is_an_integer():
    """Rule 9 and rule 15 over 200 000 pairs with ``union < 2^31``: random ones and ones within a few rows of one half."""
    rng = np.random.default_rng(0)
    union = rng.integers(1, 2 ** 31, 100000)
    inter = (rng.random(100000) * (union + 1)).astype(np.int64).clip(0, union)
    near_u = rng.integers(1, 2 ** 31, 100000)
    near_i = (near_u // 2 + rng.integers(-2, 4, 100000)).clip(0, near_u)
    union, inter = np.concatenate([union, near_u]), np.concatenate([inter, near_i])
    assert len(union) == 200000 and (union < 2 ** 31).all() and (inter <= union).all() and (2 * near_i == near_u).sum() > 1000
    q = inter.astype(np.float64) / union.astype(np.float64)         # one IEEE division each
    assert np.array_equal(2 * inter > union, q > 0.5)
    t = q * 2.0 ** 53
    m = 2 * inter > union
    assert m.sum() > 50000 and np.array_equal(t[m], np.floor(t[m]))  # every match (rule 15; a quotient BELOW 1/2 has finer bits: no integer)
    assert ((t[m] > 2.0 ** 52) & (t[m] <= 2.0 ** 53)).all()           # ... in (2^52, 2^53]
    assert np.array_equal(t[q >= 0.5], np.floor(t[q >= 0.5]))        # (and the quotients AT one half)
    assert R.iou_integer(6, 11) == (6 / 11, 0x11745D1745D174) and R.iou_integer(7, 7)[1] == 1 << 53


def test_exact_sum_and_running_fp64_sum_stay_within_the_stated_bound():
    total = 0
    for case in generated():
        table, fsum, _ = table_of(case, per_cloud=False)
        exact = R.iou_sum(table)
        assert (np.abs(exact - fsum) <= R.deviation_bound(table)).all(), (exact, fsum)
        total += int(table[:, 0].sum())
    assert total > 500                                               # (the bound was not held on empty tables)


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_worked_tables(name):
    case = R.hand_cases()[name]
    table, fsum, err = table_of(case)
    assert table.tolist() == case["table"].tolist() and err == case["err"]
    # per cloud, summed: the same table
    per, _, err2 = table_of(case, per_cloud=True)
    assert np.array_equal(per.sum(0), table) and err2 == err


# mutant -> a hand-worked case whose table it changes
KILLED_BY = {"ge_half": "iou_5_10", "area_gt_min": "min_points_4", "ignored_kept": "ignored_rows_lift", "no_class_key": "id_under_two_classes",
             "no_cloud_key": "key_in_two_clouds", "cross_class": "pair_across_classes", "no_things": "things_mask"}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_of_the_rule_changes_a_table(mutant):
    case = R.hand_cases()[KILLED_BY[mutant]]
    assert table_of(case)[0].tolist() == case["table"].tolist()
    assert table_of(case, mutant=mutant)[0].tolist() != case["table"].tolist()


def test_scores_follow_the_api_formulas():
    table = np.array([[2, 1, 1, (3 << 20) + 5, 77], [0, 0, 0, 0, 0], [0, 2, 0, 0, 0], [9, 9, 9, 9, 9]], np.int64)
    from pointnet12_amd import metrics
    s = metrics.panoptic_scores(table, include=[1, 1, 1, 0])
    iou0 = (((3 << 20) + 5 << 32) + 77) / (1 << 53)
    assert s["iou_sum"][0] == iou0 and s["tp"].tolist() == [2, 0, 0, 9] and s["fp"].tolist() == [1, 0, 2, 9]
    assert s["sq_per_class"][0] == iou0 / 2 and s["rq_per_class"][0] == 2 / 3.0 and s["pq_per_class"][0] == iou0 / 2 * (2 / 3.0)
    assert s["sq_per_class"][1] == 0 and s["rq_per_class"][1] == 0 and s["rq_per_class"][2] == 0     # the API's eps: 0 / eps
    assert s["pq"] == (s["pq_per_class"][0] + 0 + 0) / 3 and s["rq"] == (2 / 3.0) / 3
    # leading axes are summed in integers first
    both = metrics.panoptic_scores(np.stack([table, table]), include=[1, 1, 1, 0])
    assert both["tp"].tolist() == [4, 0, 0, 18] and both["iou_sum"][0] == 2 * iou0 and both["rq"] == s["rq"]


def test_split_label_words_round_trips_write_labels(tmp_path):
    rng = np.random.default_rng(3)
    sem, inst = rng.integers(0, 0x10000, 5000), rng.integers(0, 0x10000, 5000)
    sem[:4], inst[:4] = [0, 0xFFFF, 0, 0xFFFF], [0, 0, 0xFFFF, 0xFFFF]
    fn = str(tmp_path / "000000.label")
    kitti.write_labels(fn, sem, inst)
    words = np.fromfile(fn, dtype=np.uint32)
    for given in (words, torch.from_numpy(words.view(np.int32)), words.reshape(50, 100)):
        s, i = kitti.split_label_words(given, device="cpu")
        assert s.dtype == torch.int32 and i.dtype == torch.int32 and s.shape == (5000,)
        assert np.array_equal(s.numpy(), sem) and np.array_equal(i.numpy(), inst)
    kitti.write_labels(fn, sem)                                      # no instances: the high halves are 0
    s, i = kitti.split_label_words(np.fromfile(fn, dtype=np.uint32), device="cpu")
    assert np.array_equal(s.numpy(), sem) and not i.any()
    with pytest.raises(ValueError):
        kitti.split_label_words(words.astype(np.int64), device="cpu")


def test_binding_carries_the_new_symbols_and_error_bits():
    assert {"pn2_panoptic_workspace_bytes", "pn2_panoptic_count"} <= set(_lib.SIGNATURES)
    assert (_lib.PANOPTIC_ERR_CLASS, _lib.PANOPTIC_ERR_ROWS) == (R.ERR_CLASS, R.ERR_ROWS) == (256, 512)
    others = (_lib.SCAN_ERR_CLASS | _lib.SCAN_ERR_ROWS | _lib.VOXEL_ERR_RANGE | _lib.VOXEL_ERR_ROWS | _lib.SEGMENT_ERR_RANGE |
              _lib.SEGMENT_ERR_NONFINITE | _lib.CLUSTER_ERR_INDEX | _lib.CLUSTER_ERR_CELL | _lib.CLUSTER_ERR_CAP | _lib.CLUSTER_ERR_ROWS)
    assert others & (R.ERR_CLASS | R.ERR_ROWS) == 0
    lib = _lib.load()                                                # host-only calls: no GPU needed
    assert lib.pn2_panoptic_workspace_bytes(1, 0) == 3 * 64 * 16 and lib.pn2_panoptic_workspace_bytes(2, 4099) == 2 * 3 * 16384 * 16
    assert lib.pn2_panoptic_workspace_bytes(0, 10) == -1 and lib.pn2_panoptic_workspace_bytes(1, -1) == -1
    assert lib.pn2_panoptic_workspace_bytes(1, _lib.VOXEL_MAX_ROWS + 1) == -1
    assert lib.pn2_panoptic_count(None, None, None, None, None, None, 1, 8, 8, 3, None, None, 30, None, 0, None, None, None) == -1
