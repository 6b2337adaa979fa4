"""Device-side segmentation metrics: the evaluation the reference runs after every epoch (``test_semseg``, ``test_partseg``,
``test_clf``, ``calc_categorical_iou``, ``compute_cat_iou``, ``to_categorical`` of pcd_utils.py; ``test_kitti_semseg`` of pcdseg.py)
under the reference's names and argument lists, on one HIP kernel.

Everything those functions report follows from one small integer table per cloud (or per batch): how many points of true class
``t`` were predicted as class ``c``.  ``pn2_seg_confusion`` (csrc/metrics.hip) produces it in one pass over the log-probabilities
-- a row arg-max and a histogram, no host involvement -- where the reference makes ``2 C + 1`` blocking reads and ``4 C``
elementwise passes per batch.  ``SegEvaluator`` keeps the tables of a whole evaluation pass on the device and reads them back ONCE;
the reference's arithmetic is then redone on the host in the reference's own dtypes, so the reported numbers are the reference's
bit for bit:

  * ``calc_categorical_iou`` divides in float32 and adds into a float64 table (the integer 1 where the union is empty);
  * ``compute_cat_iou`` divides in float64 per cloud;
  * ``test_kitti_semseg`` adds a Python-float quotient into a float32 array per batch, starts ``count[0]`` at 1 and averages
    the classes ``1:``;
  * accuracy is the mean of per-batch quotients, never a pooled ratio.

Table layout (include/pn2.h): int64 ``[C + 1, C]``, ``conf[t, c]`` for targets in ``[0, C)``; row ``C`` collects the points whose
label is no class: the reference counts such a point in the union of the class it was predicted as and in no target set.

Differences from the reference, all deliberate: float32 log-probabilities on the GPU only (a CPU tensor raises ``Pn2Error``,
another float dtype ``RuntimeError`` -- there is no fallback path); at most 64 classes; the loops take any iterable of batches and
run the model under ``torch.no_grad()``; name grouping (``catdict``) returns a name-sorted ``dict`` instead of a pandas Series and
``test_kitti_semseg`` prints its table itself; ``compute_overall_iou`` is left out (the reference never calls it, and it compares
values with class ids).  ``confusion``, ``iou_counts``, ``SegEvaluator`` and ``ignore_index`` are additions.
"""
from collections import defaultdict

import numpy as np
import torch

from . import _lib
from ._lib import check as _check, ptr as _p

MAX_CLASSES = 64        # include/pn2.h: pn2_seg_confusion answers PN2_EUNSUPPORTED above
_NO_IGNORE = -2 ** 63


def _rows(log_probs, C):
    """log_probs [B,N,C'] or [R,C'] -> (tensor to read, B, N, row pitch): the tensor itself when its last stride is 1 and its
    rows are evenly pitched (a column slice of a padded buffer included), a contiguous copy otherwise."""
    if log_probs.dim() == 3:
        B, N = int(log_probs.shape[0]), int(log_probs.shape[1])
    elif log_probs.dim() == 2:
        B, N = 1, int(log_probs.shape[0])
    else:
        raise ValueError("log_probs must be [B, N, C] or [R, C], got %s" % (tuple(log_probs.shape),))
    if B * N == 0:
        return log_probs, B, N, max(C, 1)
    st = log_probs.stride()
    if B * N == 1:
        ld = max(C, 1)
    elif log_probs.dim() == 2 or B == 1:
        ld = st[-2]
    elif N == 1:
        ld = st[0]
    else:
        ld = st[1] if st[0] == N * st[1] else -1
    if (log_probs.shape[-1] > 1 and st[-1] != 1) or ld < C or ld >= 2 ** 31:
        log_probs = log_probs.contiguous()
        ld = int(log_probs.shape[-1])
    return log_probs, B, N, int(ld)


def confusion(log_probs, target, num_classes=None, per_cloud=False, out=None, ignore_index=None, return_pred=False):
    """Confusion table(s) of ``log_probs`` ``[B, N, C]`` (or ``[R, C]``: one cloud) against ``target`` (any integer dtype,
    ``[B, N]``, ``[B, N, 1]`` or ``[R]``): int64 ``[C + 1, C]`` pooled over the batch, ``[B, C + 1, C]`` with ``per_cloud``.

    The prediction of a row is ``log_probs.max(-1)[1]``: the lowest index on ties, the first NaN if there is one.  With ``out=``
    the counts are ADDED into ``out``.  Rows whose target equals ``ignore_index`` are skipped.  ``return_pred`` also returns the
    int64 predictions in the shape of ``target``.  Nothing is read back and nothing waits for the device: the call can be
    captured in a graph."""
    if not isinstance(log_probs, torch.Tensor) or not log_probs.is_cuda:
        raise _lib.Pn2Error("confusion: log_probs must live on the GPU: this package has no CPU path")
    if log_probs.dtype != torch.float32:
        raise RuntimeError("confusion: log_probs must be float32 (got %s)" % log_probs.dtype)
    C = int(log_probs.shape[-1]) if num_classes is None else int(num_classes)
    if not 1 <= C <= int(log_probs.shape[-1]):
        raise ValueError("confusion: num_classes = %d, log_probs has %d columns" % (C, log_probs.shape[-1]))
    if C > MAX_CLASSES:
        raise _lib.Pn2Error("confusion: %d classes are not supported (1 <= C <= %d; there is no fallback path)" % (C, MAX_CLASSES))
    if target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
        raise RuntimeError("confusion: target must have an integer dtype (got %s)" % target.dtype)
    logp, B, N, ld = _rows(log_probs.detach(), C)
    if target.numel() != B * N:
        raise ValueError("confusion: %d rows of log-probabilities, %d targets" % (B * N, target.numel()))
    tgt = target.detach().reshape(-1).to(device=logp.device, dtype=torch.int64).contiguous()
    shape = (B, C + 1, C) if per_cloud else (C + 1, C)
    if out is None:
        out = torch.zeros(shape, device=logp.device, dtype=torch.int64)
    elif (out.dtype != torch.int64 or out.device != logp.device or tuple(out.shape) != shape or not out.is_contiguous()):
        raise ValueError("confusion: out must be a contiguous int64 %s tensor on %s" % (shape, logp.device))
    pred = torch.empty(target.shape, device=logp.device, dtype=torch.int64) if return_pred else None
    ignore = _NO_IGNORE if ignore_index is None else int(ignore_index)
    if B * N > 0:
        _check(_lib.load().pn2_seg_confusion(_p(logp), ld, _p(tgt), B, N, C, ignore, _p(out), (C + 1) * C if per_cloud else 0,
                                             _p(pred), _lib.stream()), "pn2_seg_confusion")
    return (out, pred) if return_pred else out


def iou_counts(conf):
    """Table(s) ``[..., C + 1, C]`` (tensor or array) -> ``(I, U)`` int64 ``[..., C]``: per class the size of the intersection
    and of the union of {predicted as c} and {labelled c}.  ``I = diag``; ``U = column sum + row sum - I``, the column sum over
    all ``C + 1`` rows."""
    C = conf.shape[-1]
    if isinstance(conf, torch.Tensor):
        inter = torch.diagonal(conf[..., :C, :], dim1=-2, dim2=-1)
        return inter, conf.sum(-2) + conf[..., :C, :].sum(-1) - inter
    conf = np.asarray(conf)
    inter = np.diagonal(conf[..., :C, :], axis1=-2, axis2=-1)
    return inter, conf.sum(-2) + conf[..., :C, :].sum(-1) - inter


class SegEvaluator:
    """The tables of one evaluation pass, kept on the device: ``update`` writes a batch's table (``per_cloud``: its ``B``
    tables) into the next slot(s) of a tape that grows by doubling, ``tables()`` returns them all as one int64 array
    ``[slots, C + 1, C]`` -- the only synchronisation of the pass.  ``batches`` lists ``(first slot, slots, rows)`` per update."""

    def __init__(self, num_classes, per_cloud=False):
        self.num_classes = int(num_classes)
        self.per_cloud = bool(per_cloud)
        self.batches = []
        self._tape = None
        self._used = 0

    def __len__(self):
        return self._used

    def _reserve(self, k, device):
        C = self.num_classes
        if self._tape is None:
            self._tape = torch.zeros(max(16, 2 * k), C + 1, C, device=device, dtype=torch.int64)
        while self._used + k > self._tape.shape[0]:
            grown = torch.zeros(2 * self._tape.shape[0], C + 1, C, device=self._tape.device, dtype=torch.int64)
            grown[:self._used] = self._tape[:self._used]
            self._tape = grown
        return self._tape[self._used:self._used + k]

    def update(self, log_probs, target, ignore_index=None):
        if self.per_cloud and log_probs.dim() == 2:
            log_probs = log_probs.unsqueeze(0)
        k = int(log_probs.shape[0]) if self.per_cloud else 1
        if k > 0:
            slot = self._reserve(k, log_probs.device)
            confusion(log_probs, target, self.num_classes, per_cloud=self.per_cloud, out=slot if self.per_cloud else slot[0],
                      ignore_index=ignore_index)
        self.batches.append((self._used, k, int(target.numel())))
        self._used += k

    def tables(self):
        C = self.num_classes
        if self._tape is None:
            return np.zeros((0, C + 1, C), np.int64)
        return self._tape[:self._used].cpu().numpy()


# ----------------------------------------------------------------------------------------------- the reference's arithmetic, on tables
def _add_categorical_iou(table, num_classes, iou_tabel):
    """pcd_utils.py:104-112 on one pooled table: a float32 quotient (or the integer 1) added into the float64 table."""
    inter, union = iou_counts(table)
    for cat in range(num_classes):
        if union[cat] == 0:
            iou = 1
        else:
            iou = np.float32(inter[cat]) / np.float32(union[cat])
        iou_tabel[cat, 0] += iou
        iou_tabel[cat, 1] += 1
    return iou_tabel


def _add_cat_iou(tables, num_classes, iou_tabel, iou_list):
    """pcd_utils.py:82-98 on per-cloud tables: a float64 quotient (or the integer 1) per cloud and class."""
    inter, union = iou_counts(tables)
    for j in range(tables.shape[0]):
        for cat in range(num_classes):
            if union[j, cat] == 0:
                iou = 1
            else:
                iou = inter[j, cat] / float(union[j, cat])
            iou_tabel[cat, 0] += iou
            iou_tabel[cat, 1] += 1
            iou_list.append(iou)
    return iou_tabel, iou_list


def _correct(tables):
    """Rows whose prediction equals their label: the trace of the class rows, summed over the given tables."""
    C = tables.shape[-1]
    return int(np.trace(tables[..., :C, :], axis1=-2, axis2=-1).sum())


def _group_mean(values, catdict):
    """``DataFrame.groupby('Category_IOU')['mean_iou'].mean()`` of the reference without pandas: name -> mean, sorted by name."""
    groups = defaultdict(list)
    for i in range(len(catdict)):
        groups[catdict[i]].append(values[i])
    return {name: float(np.mean(groups[name])) for name in sorted(groups)}


def _check_classes(pred, num_classes):
    if pred.shape[-1] != num_classes:
        raise ValueError("the model returns %d columns for num_classes = %d" % (pred.shape[-1], num_classes))


def _first(out, index=0):
    return out[index] if isinstance(out, (tuple, list)) else out


# ----------------------------------------------------------------------------------------------- the reference's names
def to_categorical(y, num_classes):
    """1-hot encodes a tensor (pcd_utils.py:32-37), built on the device ``y`` lives on."""
    return torch.eye(num_classes, device=y.device)[y.detach().long()]


def calc_categorical_iou(pred, target, num_classes, iou_tabel):
    """pcd_utils.py:101-113: per class I / U of the whole batch (float32), added into ``iou_tabel[:, 0]``; ``[:, 1]`` counts."""
    target.squeeze_(-1)                                                    # (the reference's own side effect)
    _check_classes(pred, num_classes)
    return _add_categorical_iou(confusion(pred, target, num_classes).cpu().numpy(), num_classes, iou_tabel)


def compute_cat_iou(pred, target, num_classes, iou_tabel):
    """pcd_utils.py:79-99: per cloud and class I / U (float64) -> ``(iou_tabel, iou_list)``."""
    _check_classes(pred, num_classes)
    return _add_cat_iou(confusion(pred, target, num_classes, per_cloud=True).cpu().numpy(), num_classes, iou_tabel, [])


def test_clf(model, loader):
    """pcd_utils.py:65-77: the mean over the batches of (correct / batch size); ``pred [B, K]`` counts as B one-row clouds."""
    ev, sizes = None, []
    with torch.no_grad():
        for points, target in loader:
            target = target[:, 0]
            points = points.transpose(2, 1)
            points, target = points.cuda(), target.cuda()
            classifier = model.eval()
            pred = _first(classifier(points))
            if ev is None:
                ev = SegEvaluator(pred.shape[-1])
            ev.update(pred, target.long())
            sizes.append(points.size()[0])
    tables = ev.tables() if ev is not None else ()
    mean_correct = [_correct(tables[j]) / float(sizes[j]) for j in range(len(sizes))]
    return np.mean(mean_correct)


def test_partseg(model, loader, catdict, model_name, num_classes=50):
    """pcd_utils.py:132-175.  catdict = {0:Airplane, 1:Airplane, ...49:Table} -> ``(metrics, hist_acc, cat_iou)``."""
    iou_tabel = np.zeros((len(catdict), 3))
    iou_list = []
    metrics = defaultdict(lambda: list())
    hist_acc = []
    ev, sizes = SegEvaluator(num_classes, per_cloud=True), []
    with torch.no_grad():
        for points, label, target, norm_plt in loader:
            batchsize, num_point, _ = points.size()
            points, label, target, norm_plt = points.float(), label.long(), target.long(), norm_plt.float()
            points = points.transpose(2, 1)
            norm_plt = norm_plt.transpose(2, 1)
            points, label, target, norm_plt = points.cuda(), label.squeeze().cuda(), target.cuda(), norm_plt.cuda()
            if model_name == 'pointnet':
                seg_pred = _first(model(points, to_categorical(label, 16)), 1)
            else:
                seg_pred = _first(model(points, norm_plt, to_categorical(label, 16)))
            _check_classes(seg_pred, num_classes)
            ev.update(seg_pred.reshape(batchsize, num_point, num_classes), target)
            sizes.append(batchsize * num_point)
    tables = ev.tables()
    for (first, k, _), size in zip(ev.batches, sizes):
        iou_tabel, iou_list = _add_cat_iou(tables[first:first + k], num_classes, iou_tabel, iou_list)
        metrics['accuracy'].append(_correct(tables[first:first + k]) / size)

    iou_tabel[:, 2] = iou_tabel[:, 0] / iou_tabel[:, 1]
    hist_acc += metrics['accuracy']
    metrics['accuracy'] = np.mean(hist_acc)
    metrics['inctance_avg_iou'] = np.mean(iou_list)
    cat_iou = _group_mean(iou_tabel[:, 2], catdict)
    metrics['class_avg_iou'] = np.mean(list(cat_iou.values()))
    return metrics, hist_acc, cat_iou


def test_semseg(model, loader, catdict, model_name, num_classes):
    """pcd_utils.py:177-210 -> ``(metrics, cat_iou)`` with ``metrics['accuracy']`` and ``metrics['iou']``."""
    iou_tabel = np.zeros((len(catdict), 3))
    metrics = defaultdict(lambda: list())
    ev, sizes = SegEvaluator(num_classes), []
    with torch.no_grad():
        for points, target in loader:
            batchsize, num_point, _ = points.size()
            points, target = points.float(), target.long()
            points = points.transpose(2, 1)
            points, target = points.cuda(), target.cuda()
            pred = _first(model(points))                                   # 'pointnet' returns (pred, trans_feat)
            _check_classes(pred, num_classes)
            ev.update(pred, target)
            sizes.append(batchsize * num_point)
    tables = ev.tables()
    for j, size in enumerate(sizes):
        iou_tabel = _add_categorical_iou(tables[j], num_classes, iou_tabel)
        metrics['accuracy'].append(_correct(tables[j]) / size)

    iou_tabel[:, 2] = iou_tabel[:, 0] / iou_tabel[:, 1]
    metrics['accuracy'] = np.mean(metrics['accuracy'])
    metrics['iou'] = np.mean(iou_tabel[:, 2])
    cat_iou = _group_mean(iou_tabel[:, 2], catdict)
    return metrics, cat_iou


def test_kitti_semseg(model, loader, model_name, num_classes, class_names):
    """pcdseg.py:58-97 -> ``(acc, miou)``: per batch I / U added into a float32 array, class 0 (unlabelled) counted once more
    and left out of the mean."""
    ious = np.zeros((num_classes,), dtype=np.float32)
    count = np.zeros((num_classes,), dtype=np.uint32)
    count[0] = 1
    accuracy = []
    ev, sizes = SegEvaluator(num_classes), []
    with torch.no_grad():
        for points, target in loader:
            batch_size, num_point, _ = points.size()
            points = points.float().transpose(2, 1).cuda()
            target = target.long().cuda()
            pred = _first(model(points))
            _check_classes(pred, num_classes)
            ev.update(pred, target)
            sizes.append(batch_size * num_point)
    tables = ev.tables()
    for j, size in enumerate(sizes):
        inter, union = iou_counts(tables[j])
        for class_id in range(num_classes):
            I, U = int(inter[class_id]), int(union[class_id])
            iou = 1 if U == 0 else I / U
            ious[class_id] += iou
            count[class_id] += 1
        accuracy.append(_correct(tables[j]) / size)

    categorical_iou = ious / count
    print('categorical mIOU')
    width = max([len(str(n)) for n in class_names] + [4])
    print('%-*s  %s' % (width, '', 'mIOU'))
    for i in sorted(range(num_classes), key=lambda i: -categorical_iou[i]):
        print('%-*s  %.6f' % (width, class_names[i], categorical_iou[i]))

    acc = np.mean(accuracy)
    miou = np.mean(categorical_iou[1:])
    return acc, miou
