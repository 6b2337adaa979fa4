#!/usr/bin/env python3
"""Generate tests/golden/g16_metrics.npz by running the REFERENCE's pcd_utils.py (imported unmodified) on CPU (development
container only, like tools/make_golden_chamfer.py).  Per case <c> of ``cases``:

  <c>/logp            float32 [B, N, C]: what the model returned (values on a 1/256 grid, so the file stays small)
  <c>/target          int64 [B, N]
  <c>/nbatch          the B clouds were fed as this many equal batches
  <c>/pred            ``logp.max(-1)[1]`` as torch computed it (int64 [B, N])
  <c>/tables          int64 [B, C + 1, C] by plain counting over (target, pred): row C holds the labels that are no class
  <c>/calc_tabel      ``iou_tabel`` [C, 2] after ``calc_categorical_iou`` on every batch in turn
  <c>/cat_tabel, <c>/cat_list    ``iou_tabel`` [C, 2] and the concatenated ``iou_list`` of ``compute_cat_iou`` on every batch
  ties/expected       the lowest index among the classes that share the row maximum, written down by hand

and the reference's own loops, run with a stub model that returns the recorded log-probabilities (``Tensor.cuda`` is made the
identity while they run; their text is not touched):

  loop_semseg/*       ``test_semseg`` on case s13:  accuracy, iou, names, cat_iou
  loop_partseg/*      ``test_partseg`` on case p50: accuracy, inctance_avg_iou, class_avg_iou, hist_acc, names, cat_iou
  loop_clf/*          ``test_clf`` on case clf:     accuracy

pcdseg.py cannot be imported (open3d, cv2): its aggregation is restated in tests/metrics_ref.py.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_metrics.py
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PN2_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pcd_utils as R                   # noqa: E402  (the reference)
import metrics_ref as M                 # noqa: E402  (this project's restatement)

OUT = os.path.join(ROOT, "tests", "golden", "g16_metrics.npz")

S3DIS = ["ceiling", "floor", "wall", "beam", "column", "window", "door", "table", "chair", "sofa", "bookcase", "board", "clutter"]
# ShapeNet-part: the 50 part ids belong to 16 categories in runs of these lengths
PARTS = [("Airplane", 4), ("Bag", 2), ("Cap", 2), ("Car", 4), ("Chair", 4), ("Earphone", 3), ("Guitar", 3), ("Knife", 2), ("Lamp", 4),
         ("Laptop", 2), ("Motorbike", 6), ("Mug", 2), ("Pistol", 3), ("Rocket", 3), ("Skateboard", 3), ("Table", 3)]
PART_NAMES = [name for name, n in PARTS for _ in range(n)]


class cuda_is_identity:
    def __enter__(self):
        self._orig = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self

    def __exit__(self, *exc):
        torch.Tensor.cuda = self._orig
        return False


def coherent_labels(rng, B, N, choices):
    """Labels in runs of 8 .. 200 equal values, as the points of a scanned surface come; choices[b] = the ids cloud b may hold."""
    out = np.empty((B, N), np.int64)
    for b in range(B):
        n = 0
        while n < N:
            run = int(rng.integers(8, 200))
            out[b, n:n + run] = rng.choice(choices[b])
            n += run
    return out


def scores(rng, target, C, bonus=3.0):
    """Log-probability-like scores on a 1/256 grid in [-16, 0]: the labelled class is favoured, ties happen by themselves."""
    B, N = target.shape
    x = -rng.integers(0, 4097, size=(B, N, C)).astype(np.float32) / 256
    ok = (target >= 0) & (target < C)
    b, n = np.nonzero(ok)
    x[b, n, target[b, n]] = np.minimum(0.0, x[b, n, target[b, n]] / 4 + np.float32(bonus) / 256)
    return x.astype(np.float32)


def record(out, name, logp, target, nbatch):
    logp = np.ascontiguousarray(logp, np.float32)
    target = np.ascontiguousarray(target, np.int64)
    B, N, C = logp.shape
    assert B % nbatch == 0
    pred = torch.from_numpy(logp).max(-1)[1].numpy()
    assert np.array_equal(pred, M.argmax_lowest(logp)), name            # torch's arg-max IS lowest-index / first-NaN
    assert np.array_equal(pred, torch.from_numpy(logp).argmax(-1).numpy()), name
    calc_tabel, cat_tabel, cat_list = np.zeros((C, 3)), np.zeros((C, 3)), []
    for lp, tg in zip(np.split(logp, nbatch), np.split(target, nbatch)):
        calc_tabel = R.calc_categorical_iou(torch.from_numpy(lp.copy()), torch.from_numpy(tg.copy()), C, calc_tabel)
        cat_tabel, lst = R.compute_cat_iou(torch.from_numpy(lp.copy()), torch.from_numpy(tg.copy()), C, cat_tabel)
        cat_list += lst
    out[name + "/logp"], out[name + "/target"], out[name + "/nbatch"] = logp, target, np.int64(nbatch)
    out[name + "/pred"] = pred.astype(np.int64)
    out[name + "/tables"] = M.count_tables(pred, target, C)
    out[name + "/calc_tabel"] = calc_tabel[:, :2].copy()
    out[name + "/cat_tabel"] = cat_tabel[:, :2].copy()
    out[name + "/cat_list"] = np.array(cat_list, np.float64)


class Stub:
    """A 'model' that returns the recorded log-probabilities batch by batch, wrapped the way each family returns them."""

    def __init__(self, batches, wrap):
        self.batches, self.wrap, self.i = batches, wrap, 0

    def eval(self):
        return self

    def __call__(self, *args):
        lp = torch.from_numpy(self.batches[self.i].copy())
        self.i += 1
        return self.wrap(lp)


def main():
    rng = np.random.default_rng(16)
    out, cases = {}, []

    def add(name):
        cases.append(name)
        return name

    t = coherent_labels(rng, 3, 1024, [np.arange(13)] * 3)
    t[2][t[2] == 5] = 6                                   # class 5 is absent from cloud 2's labels
    record(out, add("s13"), scores(rng, t, 13), t, 3)
    t = coherent_labels(rng, 2, 2048, [np.arange(20), np.arange(1, 17)])
    record(out, add("k20"), scores(rng, t, 20), t, 2)
    starts = np.cumsum([0] + [n for _, n in PARTS])
    cats = [0, 4, 10, 15]                                 # one category per cloud: its parts are the only labels
    t = coherent_labels(rng, 4, 512, [np.arange(starts[c], starts[c + 1]) for c in cats])
    x = scores(rng, t, 50)
    for b, c in enumerate(cats):                          # the network knows the category: other categories' parts score low
        x[b, :, :starts[c]] -= 32
        x[b, :, starts[c + 1]:] -= 32
    x[0, :40, 30] = 1.0                                   # ... except for a few stray predictions
    record(out, add("p50"), x, t, 2)

    # ties: the row maximum shared by two or three classes, exact float32 constants, the lowest index expected
    vals = [-0.5, -0.125, 0.0, -1.0, -2.25, -0.0078125]
    rows, expect, tt = [], [], []
    for i in range(128):
        C = 8
        top = np.float32(vals[i % len(vals)])
        row = np.full(C, top - np.float32(1 + (i % 5)), np.float32)
        first = i % 6
        others = [first + 1 + (i // 6) % (C - first - 1)]
        if i % 2:
            k = first + 1 + (i // 12 + 3) % (C - first - 1)
            if k not in others:
                others.append(k)
        for k in [first] + others:
            row[k] = top
        rows.append(row)
        expect.append(first)
        tt.append((i * 3) % C)
    x = np.stack(rows)[None]
    record(out, add("ties"), x, np.array(tt, np.int64)[None], 1)
    out["ties/expected"] = np.array(expect, np.int64)[None]
    assert np.array_equal(out["ties/pred"], out["ties/expected"])
    assert -0.0 == 0.0 and sum(1 for r in rows if (r == r.max()).sum() == 3) >= 20

    # NaN rows, rows of all -inf, labels -1, C and 255
    t = coherent_labels(rng, 2, 64, [np.arange(13)] * 2)
    x = scores(rng, t, 13)
    x[0, 0, 7] = np.nan
    x[0, 1, [3, 9]] = np.nan                              # the first NaN wins
    x[0, 2, 12] = np.nan
    x[0, 2, 0] = 0.0                                      # ... over a larger finite value in front of it
    x[0, 3, :] = -np.inf
    x[1, 5, :] = -np.inf
    x[1, 6, :] = np.nan
    x[1, 7, 1:] = -np.inf
    x[1, 8, :12] = -np.inf
    x[1, 9, 4] = np.inf
    t[0, [0, 10, 11]] = -1
    t[0, [3, 20, 21, 22]] = 13
    t[1, [5, 30, 31]] = 255
    t[1, 40] = -100
    t[1, 41] = 2 ** 40
    record(out, add("special"), x, t, 1)
    assert out["special/pred"][0, :4].tolist() == [7, 3, 12, 0] and out["special/pred"][1, 5:10].tolist() == [0, 0, 0, 12, 4]

    t = np.zeros((2, 32), np.int64)
    t[0, [3, 4]] = 1
    t[1, 7] = -1
    record(out, add("c1"), -rng.integers(0, 9, size=(2, 32, 1)).astype(np.float32) / 256, t, 2)
    assert not out["c1/pred"].any()

    t = rng.integers(0, 40, size=(3, 8))                  # three classifier batches of eight shapes: [8, 40] each
    record(out, add("clf"), scores(rng, t, 40, bonus=40.0), t, 3)

    # ---- the reference's own loops over the recorded batches
    def batches(c):
        n = int(out[c + "/nbatch"])
        return np.split(out[c + "/logp"], n), np.split(out[c + "/target"], n)

    with cuda_is_identity():
        lps, tgs = batches("s13")
        loader = [(torch.zeros(lp.shape[0], lp.shape[1], 6), torch.from_numpy(tg.copy())) for lp, tg in zip(lps, tgs)]
        metrics, cat_iou = R.test_semseg(Stub(lps, lambda lp: lp), loader, dict(enumerate(S3DIS)), "pointnet2", 13)
        out["loop_semseg/accuracy"], out["loop_semseg/iou"] = np.float64(metrics["accuracy"]), np.float64(metrics["iou"])
        out["loop_semseg/names"], out["loop_semseg/cat_iou"] = np.array(list(cat_iou.index)), cat_iou.to_numpy(np.float64)
        metrics_v1, _ = R.test_semseg(Stub(lps, lambda lp: (lp, None)), loader, dict(enumerate(S3DIS)), "pointnet", 13)
        assert metrics_v1["iou"] == metrics["iou"]

        lps, tgs = batches("p50")
        loader = [(torch.zeros(lp.shape[0], lp.shape[1], 3), torch.zeros(lp.shape[0], 1, dtype=torch.int64), torch.from_numpy(tg.copy()),
                   torch.zeros(lp.shape[0], lp.shape[1], 3)) for lp, tg in zip(lps, tgs)]
        metrics, hist_acc, cat_iou = R.test_partseg(Stub(lps, lambda lp: lp), loader, dict(enumerate(PART_NAMES)), "pointnet2", 50)
        for k in ("accuracy", "inctance_avg_iou", "class_avg_iou"):
            out["loop_partseg/" + k] = np.float64(metrics[k])
        out["loop_partseg/hist_acc"] = np.array(hist_acc, np.float64)
        out["loop_partseg/names"], out["loop_partseg/cat_iou"] = np.array(list(cat_iou.index)), cat_iou.to_numpy(np.float64)

        lps, tgs = batches("clf")
        loader = [(torch.zeros(lp.shape[1], 16, 3), torch.from_numpy(tg[0][:, None].copy())) for lp, tg in zip(lps, tgs)]
        out["loop_clf/accuracy"] = np.float64(R.test_clf(Stub([lp[0] for lp in lps], lambda lp: (lp, None)), loader))

    out["s3dis_names"], out["part_names"] = np.array(S3DIS), np.array(PART_NAMES)
    out["cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1000000, size
    print("wrote %s (%d bytes), cases: %s" % (OUT, size, " ".join(cases)))
    for c in cases:
        tb = out[c + "/tables"].sum(0)
        print("  %-8s logp %-16s batches %d  accuracy %.3f  out-of-range labels %d  classes with U == 0 (pooled) %d" % (
            c, out[c + "/logp"].shape, out[c + "/nbatch"], np.trace(tb[:-1]) / tb.sum(), tb[-1].sum(),
            int(((tb.sum(0) + tb[:-1].sum(1)) == 0).sum())))


if __name__ == "__main__":
    main()
