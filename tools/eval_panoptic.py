#!/usr/bin/env python3
"""Panoptic quality (PQ / SQ / RQ) of predicted ``.label`` files against the ground truth, on the HIP library
(``metrics.PanopticEvaluator`` -> ``pn2_panoptic_count``): every pair of files is uploaded as it is, the counts stay on the device,
ONE read-back at the end.

    python tools/eval_panoptic.py --pred DIR --gt DIR --config semantic-kitti.yaml [--min-points 30] [--things 1,2,3,4,5,6,7,8]
    python tools/eval_panoptic.py                      # no directories: a synthetic pair, so that it runs anywhere with the GPU

``--pred`` / ``--gt``: directories of ``%06d.label`` files with the same names (what ``kitti.write_labels(fn, scan_labels,
scan_instances)`` writes: the raw semantic id in the low 16 bits, the instance in the high 16, 0 = no instance on the PREDICTED side;
the ground truth's ids are taken as they are).  ``--config``: the dataset's yaml; its ``learning_map`` turns raw ids into the
evaluated classes, class 0 ("unlabeled") is ignored, ``--things`` names the classes whose instance ids count (the others are one
segment each).  The rule is the one of include/pn2.h, written from memory of the SemanticKITTI API and UNVERIFIED against it; PQ-dagger
and the API's semantic IoU are not computed here.  Prints the per-class table and one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                          # noqa: E402

from pointnet12_amd import kitti, metrics             # noqa: E402

CLASSES = 20                                          # SemanticKITTI's learning_map: 0 = unlabeled, 1 .. 19
THINGS = (1, 2, 3, 4, 5, 6, 7, 8)


def synthetic_pair(seed, n, classes=CLASSES, things=THINGS, instances=120):
    """A scan-shaped pair of labellings, ``(pred_sem, pred_inst, gt_sem, gt_inst)`` int32 ``[n]`` with class ids (not raw ids) and -1
    for "no instance": rows come in runs of one segment, as a rotating scanner delivers them; a few stuff classes own most rows
    (ONE segment of tens of thousands of rows each), ``instances`` things share the rest, 3 % of the runs are unlabeled.  The
    prediction follows the truth with shifted borders, relabelled runs, split and renamed instances and 2 % of salt."""
    rng = np.random.default_rng(seed)
    stuff = [c for c in range(1, classes) if c not in things]
    weight = np.array([0.30, 0.22, 0.15, 0.08] + [0.25 / max(len(stuff) - 4, 1)] * (len(stuff) - 4))[:len(stuff)]
    seg_cls = np.concatenate([[0], stuff, rng.choice(things, instances)])
    seg_id = np.concatenate([[0], np.zeros(len(stuff), np.int64), 1 + np.arange(instances)])
    p = np.concatenate([[0.03], 0.72 * weight / weight.sum(), np.full(instances, 0.25 / instances)])
    lengths = rng.geometric(1 / 60.0, size=n // 20 + 8)
    runs = rng.choice(len(seg_cls), size=len(lengths), p=p / p.sum())
    row_seg = np.repeat(runs, lengths)[:n]
    assert len(row_seg) == n
    gt_sem, gt_inst = seg_cls[row_seg], seg_id[row_seg]
    pred_cls, pred_id = seg_cls.copy(), np.where(seg_id > 0, seg_id + 500, 0)
    wrong = rng.random(len(seg_cls)) < 0.1                            # an instance under another class
    pred_cls[wrong] = rng.integers(1, classes, int(wrong.sum()))
    pred_run = np.repeat(runs, lengths)[:n]
    pred_run = np.roll(pred_run, 2)                                   # every border two rows late
    pred_sem, pred_inst = pred_cls[pred_run], pred_id[pred_run]
    split = np.repeat(rng.random(len(lengths)) < 0.15, lengths)[:n] & (pred_inst > 0)
    pred_inst = np.where(split, pred_inst + 1000, pred_inst)          # some runs of an instance under an id of their own
    salt = rng.random(n) < 0.02
    pred_sem = np.where(salt, rng.integers(1, classes, n), pred_sem)
    is_thing = np.isin(pred_sem, things)
    pred_inst = np.where(is_thing & (pred_inst > 0), pred_inst, -1)
    gt_inst = np.where(np.isin(gt_sem, things), gt_inst, 0)
    return tuple(a.astype(np.int32) for a in (pred_sem, pred_inst, gt_sem, gt_inst))


def class_masks(classes, things):
    include = np.ones(classes, np.int32)
    include[0] = 0
    th = np.zeros(classes, np.int32)
    th[list(things)] = 1
    return include, th


def report(scores, include, names=None):
    width = max([len(str(n)) for n in (names or {}).values()] + [5])
    print("%-*s  %8s %8s %8s  %6s %6s %6s" % (width, "class", "PQ", "SQ", "RQ", "tp", "fp", "fn"))
    for c in np.flatnonzero(include):
        print("%-*s  %8.4f %8.4f %8.4f  %6d %6d %6d" % (width, (names or {}).get(int(c), c), scores["pq_per_class"][c], scores["sq_per_class"][c],
                                                        scores["rq_per_class"][c], scores["tp"][c], scores["fp"][c], scores["fn"][c]))
    print("%-*s  %8.4f %8.4f %8.4f" % (width, "mean", scores["pq"], scores["sq"], scores["rq"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred")
    ap.add_argument("--gt")
    ap.add_argument("--config")
    ap.add_argument("--min-points", type=int, default=30)
    ap.add_argument("--things", default=",".join(str(c) for c in THINGS))
    ap.add_argument("--rows", type=int, default=120000, help="rows of the synthetic pair")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_panoptic.py needs the GPU: the HIP library is the only implementation")
    dev = torch.device("cuda")
    things = [int(c) for c in args.things.split(",") if c != ""]
    names = None
    if args.pred is None and args.gt is None:
        include, th = class_masks(CLASSES, things)
        ev = metrics.PanopticEvaluator(CLASSES, include, th, args.min_points, device=dev)
        ev.update(*[torch.from_numpy(a).to(dev) for a in synthetic_pair(args.seed, args.rows, CLASSES, things)])
        scans = 1
    else:
        if not (args.pred and args.gt and args.config):
            sys.exit("--pred, --gt and --config go together")
        import yaml
        cfg = yaml.safe_load(open(args.config))
        lmap = {int(k): int(v) for k, v in cfg["learning_map"].items()}
        classes = max(lmap.values()) + 1
        lut = np.full(max(lmap) + 1, -1, np.int32)
        for k, v in lmap.items():
            lut[k] = v
        lut_d = torch.from_numpy(lut).to(dev)
        inv = {int(k): int(v) for k, v in cfg.get("learning_map_inv", {}).items()}
        names = {c: cfg.get("labels", {}).get(inv.get(c), c) for c in range(classes)}
        include, th = class_masks(classes, things)
        ev = metrics.PanopticEvaluator(classes, include, th, args.min_points, device=dev)
        files = sorted(f for f in os.listdir(args.gt) if f.endswith(".label"))
        if not files:
            sys.exit("no .label files in %s" % args.gt)
        for f in files:
            pred = np.fromfile(os.path.join(args.pred, f), dtype=np.uint32)
            gt = np.fromfile(os.path.join(args.gt, f), dtype=np.uint32)
            if pred.shape != gt.shape:
                sys.exit("%s: %d predicted words, %d ground-truth words" % (f, pred.size, gt.size))
            sem, inst = kitti.split_label_words(pred, dev)
            ev.update_scan(sem, inst, gt, lut_d)
        scans = len(files)
    scores = ev.scores()                                             # the one read-back
    ev.check()
    report(scores, include, names)
    print(json.dumps({"scans": scans, "min_points": args.min_points, "pq": scores["pq"], "sq": scores["sq"], "rq": scores["rq"],
                      "tp": int(scores["tp"].sum()), "fp": int(scores["fp"].sum()), "fn": int(scores["fn"].sum())}))


if __name__ == "__main__":
    main()
