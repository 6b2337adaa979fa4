"""Host restatement of the reference's evaluation arithmetic over INTEGER confusion tables (numpy only), the yardstick of
tests/test_metrics_gpu.py.  tests/test_metrics_cpu.py holds it bit for bit against what the reference itself returned
(tests/golden/g16_metrics.npz, recorded by tools/make_golden_metrics.py from the unmodified pcd_utils.py).

A table is int64 [C + 1, C]: table[t, c] = rows with label t predicted as c; row C collects the rows whose label is no class.
The reference's per-class sets then have the sizes
    I = |pred == c  and  target == c| = table[c, c]
    U = |pred == c  or   target == c| = (column c over all C + 1 rows) + (row c) - I.
pcdseg.py cannot be imported without open3d / cv2 and its loop calls .cuda(): its aggregation is restated here line by line
(test_kitti_semseg below), as are the loops of pcd_utils.py around the two per-batch functions.
"""
import math
from collections import defaultdict

import numpy as np


def argmax_lowest(x):
    """Row arg-max of [..., C] without np.argmax on the values: the first NaN if the row has one, else the first position that
    holds the row's maximum (so a row of all -inf gives 0)."""
    x = np.asarray(x)
    isn = np.isnan(x)
    top = np.where(isn, -np.inf, x).max(-1, keepdims=True)
    first_top = (x == top).argmax(-1)                     # argmax of booleans: the first True
    return np.where(isn.any(-1), isn.argmax(-1), first_top).astype(np.int64)


def count_tables(pred, target, C, ignore_index=None):
    """Plain counting: pred, target [B, N] -> int64 [B, C + 1, C]."""
    pred, target = np.asarray(pred).astype(np.int64), np.asarray(target).astype(np.int64)
    B = pred.shape[0]
    out = np.zeros((B, C + 1, C), np.int64)
    for b in range(B):
        p, t = pred[b].reshape(-1), target[b].reshape(-1)
        if ignore_index is not None:
            keep = t != ignore_index
            p, t = p[keep], t[keep]
        row = np.where((t >= 0) & (t < C), t, C)
        np.add.at(out[b], (row, p), 1)
    return out


def iou_counts(table):
    C = table.shape[-1]
    inter = np.array([table[c, c] for c in range(C)], np.int64)
    union = np.array([table[:, c].sum() + table[c, :].sum() - table[c, c] for c in range(C)], np.int64)
    return inter, union


def correct(table):
    return int(sum(int(table[c, c]) for c in range(table.shape[-1])))


def calc_categorical_iou(table, num_classes, iou_tabel):
    """pcd_utils.py:101-113 on the pooled table of one batch: `torch.sum(...).float()` twice, a float32 division read back as a
    0-dim float32 array, added into the float64 table; the integer 1 where U == 0."""
    inter, union = iou_counts(table)
    for cat in range(num_classes):
        I, U = np.float32(int(inter[cat])), np.float32(int(union[cat]))           # :105-106
        if U == 0:
            iou = 1                                                               # :108
        else:
            iou = np.asarray(I / U)                                               # :110
        iou_tabel[cat, 0] += iou                                                  # :111
        iou_tabel[cat, 1] += 1
    return iou_tabel


def compute_cat_iou(tables, num_classes, iou_tabel):
    """pcd_utils.py:79-99 on the per-cloud tables of one batch -> (iou_tabel, iou_list)."""
    iou_list = []
    for j in range(len(tables)):                                                  # :82
        inter, union = iou_counts(tables[j])
        for cat in range(num_classes):
            I, U = np.int64(inter[cat]), np.int64(union[cat])                     # :90-91 (np.sum of booleans)
            if U == 0:
                iou = 1                                                           # :93
            else:
                iou = I / float(U)                                                # :95
            iou_tabel[cat, 0] += iou
            iou_tabel[cat, 1] += 1
            iou_list.append(iou)
    return iou_tabel, iou_list


def group_mean(values, catdict):
    """groupby(name).mean() (pcd_utils.py:170-172, :206-208) with an exactly rounded sum: {name: mean}, sorted by name."""
    groups = defaultdict(list)
    for i in range(len(catdict)):
        groups[str(catdict[i])].append(float(values[i]))
    return {name: math.fsum(groups[name]) / len(groups[name]) for name in sorted(groups)}


def test_semseg(batch_tables, batch_points, catdict, num_classes):
    """pcd_utils.py:177-210 -> (accuracy, iou, cat_iou, iou_tabel); batch_points[j] = batchsize * num_point of batch j."""
    iou_tabel = np.zeros((len(catdict), 3))                                        # :178
    accuracy = []
    for table, points in zip(batch_tables, batch_points):
        iou_tabel = calc_categorical_iou(table, num_classes, iou_tabel)           # :193
        accuracy.append(correct(table) / points)                                  # :199-200
    iou_tabel[:, 2] = iou_tabel[:, 0] / iou_tabel[:, 1]                            # :202
    return np.mean(accuracy), np.mean(iou_tabel[:, 2]), group_mean(iou_tabel[:, 2], catdict), iou_tabel
test_semseg.__test__ = False


def test_partseg(batch_tables, batch_points, catdict, num_classes=50):
    """pcd_utils.py:132-175 -> (metrics dict, hist_acc, cat_iou); batch_tables[j] = the per-cloud tables of batch j."""
    iou_tabel = np.zeros((len(catdict), 3))                                        # :134
    iou_list, hist_acc = [], []
    for tables, points in zip(batch_tables, batch_points):
        iou_tabel, iou = compute_cat_iou(tables, num_classes, iou_tabel)          # :155
        iou_list += iou
        hist_acc.append(sum(correct(t) for t in tables) / points)                 # :161-162
    iou_tabel[:, 2] = iou_tabel[:, 0] / iou_tabel[:, 1]                            # :164
    cat_iou = group_mean(iou_tabel[:, 2], catdict)
    metrics = {"accuracy": np.mean(hist_acc), "inctance_avg_iou": np.mean(iou_list),
               "class_avg_iou": math.fsum(cat_iou.values()) / len(cat_iou)}       # :166-173
    return metrics, hist_acc, cat_iou
test_partseg.__test__ = False


def test_clf(batch_tables, batch_sizes):
    """pcd_utils.py:65-77: the mean over batches of correct / batch size."""
    return np.mean([correct(t) / float(n) for t, n in zip(batch_tables, batch_sizes)])
test_clf.__test__ = False


def test_kitti_semseg(batch_tables, batch_points, num_classes):
    """pcdseg.py:59-97 -> (acc, miou, categorical_iou)."""
    ious = np.zeros((num_classes,), dtype=np.float32)                              # :59
    count = np.zeros((num_classes,), dtype=np.uint32)                              # :60
    count[0] = 1                                                                   # :61
    accuracy = []
    for table, points in zip(batch_tables, batch_points):
        inter, union = iou_counts(table)
        for class_id in range(num_classes):
            I, U = int(inter[class_id]), int(union[class_id])                     # :79-80 (.cpu().item())
            iou = 1 if U == 0 else I / U                                          # :81
            ious[class_id] += iou                                                 # :82
            count[class_id] += 1                                                  # :83
        accuracy.append(correct(table) / points)                                  # :85-86
    categorical_iou = ious / count                                                 # :88
    return np.mean(accuracy), np.mean(categorical_iou[1:]), categorical_iou      # :95-96
test_kitti_semseg.__test__ = False


def ulps(a, b):
    """Distance of two float64 numbers in units in the last place of the larger one."""
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    return abs(a - b) / math.ulp(max(abs(a), abs(b)))
