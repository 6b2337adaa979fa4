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


# ----------------------------------------------------------------------------------------------- panoptic quality (csrc/panoptic.hip)
# PQ / SQ / RQ of instance labels (``VoxelGrid.components``, ``label_scan(..., instances=)``) against a ground truth.  The rule is the
# one of include/pn2.h ("panoptic quality"): WRITTEN FROM MEMORY OF THE SEMANTICKITTI API'S ``PanopticEval`` AND UNVERIFIED AGAINST IT.
# ``pn2_panoptic_count`` adds per class the integers tp, fp, fn and the two halves of the exact IoU sum into a table on the device;
# ``panoptic_scores`` does the API's few divisions on the host.  One stated deviation: the API adds the IoUs in fp64 scan by scan, here
# the sum is exact and rounded once (they differ by at most ``tp * 2^-52`` of the sum).
PANOPTIC_COLUMNS = ("tp", "fp", "fn", "iou_hi", "iou_lo")
_PANOPTIC_EPS = 1e-15                                                    # the API's
_panoptic_const = {}                                                     # (what, device, ...) -> a small constant device tensor


def _const(key, make):
    t = _panoptic_const.get(key)
    if t is None:
        t = _panoptic_const[key] = make()
    return t


def _class_mask(mask, C, device, what):
    """None -> None; an int32 ``[C]`` device tensor as it is; anything else (a list, a bool tensor) uploaded as one."""
    if mask is None:
        return None
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.int32 and mask.device == device and mask.is_contiguous():
        m = mask
    else:
        m = torch.as_tensor(np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(np.int32)).to(device)
    if m.dim() != 1 or m.numel() != C:
        raise ValueError("panoptic_counts: %s must have one entry per class (%d), got %s" % (what, C, tuple(m.shape)))
    return m


def panoptic_workspace(B, max_rows, device="cuda"):
    """The ``work=`` buffer of ``panoptic_counts`` for calls of ``B`` clouds of at most ``max_rows`` rows each."""
    nbytes = _lib.workspace_bytes("pn2_panoptic_workspace_bytes", (int(B), int(max_rows)), _lib.Pn2Error,
                                  "panoptic_workspace: B = %d, max_rows = %d are not supported" % (B, max_rows))
    return torch.empty(max(int(nbytes), 16), device=device, dtype=torch.uint8)


def panoptic_counts(pred_sem, pred_inst, gt_sem, gt_inst, num_classes, include=None, things=None, min_points=30, row_begin=None,
                    row_count=None, max_rows=None, per_cloud=False, out=None, err=None, work=None):
    """The panoptic table of predicted ``(pred_sem, pred_inst)`` against ``(gt_sem, gt_inst)``: int64 ``[C, 5]`` pooled over the
    clouds, ``[B, C, 5]`` with ``per_cloud``; columns ``tp, fp, fn, iou_hi, iou_lo`` (``panoptic_scores`` reads them).

    The four inputs are integer device tensors of one shape: ``[N]`` (one cloud), ``[B, N]`` (B clouds), or flat with
    ``row_begin`` / ``row_count`` (int64 ``[B]`` DEVICE tensors, clouds back to back as ``ScanFilter.filter`` takes them; ``max_rows``:
    a host bound of every count, None: all rows).  A negative instance id means "no segment"; ``include`` (``[C]``, None: every
    class) names the evaluated classes -- a row whose ``gt_sem`` is excluded leaves BOTH sides -- and ``things`` (``[C]`` or None)
    the classes whose ids count; the ids of the others are taken as 0, one segment per stuff class.  A ``gt_sem`` outside ``[0, C)``
    drops the row and sets ``_lib.PANOPTIC_ERR_CLASS`` in ``err`` (int32 ``[1]`` device tensor, caller zeroes, may be None); a cloud
    whose rows leave the tensors is skipped whole (``PANOPTIC_ERR_ROWS``).

    The counts are ADDED into ``out``.  With int32 inputs, ``out=``, ``work=`` (``panoptic_workspace``) and int32 device masks the call
    allocates nothing and reads nothing back: it can be captured in a graph, and a captured call stays valid when the content of
    ``row_count`` changes.  The table is the same from run to run and under any permutation of a cloud's rows, byte for byte."""
    tensors = (pred_sem, pred_inst, gt_sem, gt_inst)
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.Pn2Error("panoptic_counts: the labels must live on the GPU: this package has no CPU path")
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise RuntimeError("panoptic_counts: the labels must have an integer dtype (got %s)" % t.dtype)
        if t.shape != gt_sem.shape:
            raise ValueError("panoptic_counts: the four label tensors must have one shape")
    C, dev = int(num_classes), gt_sem.device
    if C < 1:
        raise ValueError("panoptic_counts: num_classes = %d" % C)
    if (row_begin is None) != (row_count is None):
        raise ValueError("panoptic_counts: row_begin and row_count go together")
    rows = int(gt_sem.numel())
    if row_begin is not None:
        if gt_sem.dim() != 1:
            raise ValueError("panoptic_counts: with row_begin / row_count the labels are flat [rows] tensors")
        B = int(row_begin.numel())
        for t in (row_begin, row_count):
            if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
                raise ValueError("panoptic_counts: row_begin and row_count must be int64 [B] device tensors")
        max_rows = rows if max_rows is None else int(max_rows)
    elif gt_sem.dim() == 2:
        B, N = int(gt_sem.shape[0]), int(gt_sem.shape[1])
        row_begin = _const(("begin", dev, B, N), lambda: torch.arange(B, device=dev, dtype=torch.int64) * N)
        row_count = _const(("count", dev, B, N), lambda: torch.full((B,), N, device=dev, dtype=torch.int64))
        max_rows = N
    elif gt_sem.dim() == 1:
        B = 1
        row_begin = _const(("begin", dev, 1, rows), lambda: torch.zeros(1, device=dev, dtype=torch.int64))
        row_count = _const(("count", dev, 1, rows), lambda: torch.full((1,), rows, device=dev, dtype=torch.int64))
        max_rows = rows
    else:
        raise ValueError("panoptic_counts: labels must be [N], [B, N] or flat with row_begin / row_count, got %s" % (tuple(gt_sem.shape),))
    shape = (B, C, 5) if per_cloud else (C, 5)
    if out is None:
        out = torch.zeros(shape, device=dev, dtype=torch.int64)
    elif out.dtype != torch.int64 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("panoptic_counts: out must be a contiguous int64 %s tensor on %s" % (shape, dev))
    if B == 0:
        return out
    flat = [t.detach().reshape(-1).to(torch.int32).contiguous() for t in tensors]       # (int32 contiguous tensors pass as they are)
    include = _const(("ones", dev, C), lambda: torch.ones(C, device=dev, dtype=torch.int32)) if include is None else \
        _class_mask(include, C, dev, "include")
    things = _class_mask(things, C, dev, "things")
    if err is not None and (err.dtype != torch.int32 or err.device != dev or err.numel() < 1):
        raise ValueError("panoptic_counts: err must be an int32 device tensor")
    lib = _lib.load()
    need = _lib.workspace_bytes("pn2_panoptic_workspace_bytes", (B, max_rows), _lib.Pn2Error,
                                "panoptic_counts: B = %d, max_rows = %d are not supported" % (B, max_rows))
    if work is None:
        work = panoptic_workspace(B, max_rows, dev)
    elif work.dtype != torch.uint8 or work.device != dev or work.numel() < need or not work.is_contiguous():
        raise ValueError("panoptic_counts: work must be a uint8 device tensor of at least %d bytes (panoptic_workspace)" % need)
    _check(lib.pn2_panoptic_count(_p(flat[0]), _p(flat[1]), _p(flat[2]), _p(flat[3]), _p(row_begin), _p(row_count), B, max_rows, rows, C,
                                  _p(include), _p(things), int(min_points), _p(out), 5 * C if per_cloud else 0, _p(err), _p(work),
                                  _lib.stream()), "pn2_panoptic_count")
    return out


def panoptic_scores(table, include=None):
    """The scores of a panoptic table (tensor or array ``[C, 5]``; leading axes -- clouds, updates -- are summed first), on the host
    in fp64 with the API's ``eps = 1e-15``: ``sq = iou / max(tp, eps)``, ``rq = tp / max(tp + 0.5 fp + 0.5 fn, eps)``,
    ``pq = sq * rq``, and their means over the included classes (``include``: ``[C]``, None: all).  Returns a dict with ``pq``,
    ``sq``, ``rq``, ``pq_per_class``, ``sq_per_class``, ``rq_per_class``, ``tp``, ``fp``, ``fn`` (int64 ``[C]``) and ``iou_sum``
    (fp64 ``[C]``): per class the integer ``iou_hi * 2^32 + iou_lo`` over ``2^53``, one correctly rounded division of the EXACT sum of
    the matches' fp64 IoUs."""
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.ndim < 2 or t.shape[-1] != 5:
        raise ValueError("panoptic_scores: the table must be [..., C, 5], got %s" % (t.shape,))
    t = t.astype(np.int64).reshape(-1, t.shape[-2], 5)
    C = t.shape[1]
    totals = [[sum(int(v) for v in t[:, c, k]) for k in range(5)] for c in range(C)]       # Python integers: no overflow, no order
    tp, fp, fn = (np.array([r[k] for r in totals], np.int64) for k in range(3))
    iou = np.array([((r[3] << 32) + r[4]) / (1 << 53) for r in totals], np.float64)          # int / int: correctly rounded
    inc = np.ones(C, bool) if include is None else \
        np.asarray(include.cpu() if isinstance(include, torch.Tensor) else include).reshape(-1) != 0
    if inc.shape[0] != C:
        raise ValueError("panoptic_scores: include must have one entry per class (%d)" % C)
    tpf, fpf, fnf = tp.astype(np.float64), fp.astype(np.float64), fn.astype(np.float64)
    sq = iou / np.maximum(tpf, _PANOPTIC_EPS)
    rq = tpf / np.maximum(tpf + 0.5 * fpf + 0.5 * fnf, _PANOPTIC_EPS)
    pq = sq * rq
    mean = lambda v: float(v[inc].mean()) if inc.any() else 0.0
    return {"pq": mean(pq), "sq": mean(sq), "rq": mean(rq), "pq_per_class": pq, "sq_per_class": sq, "rq_per_class": rq,
            "tp": tp, "fp": fp, "fn": fn, "iou_sum": iou}


class PanopticEvaluator:
    """The panoptic table of one evaluation pass, kept on the device (modelled on ``SegEvaluator``): every ``update`` ADDS a batch's
    counts into it -- with ``per_cloud`` each cloud gets a table of its own on a tape that grows by doubling -- and ``tables()``
    reads it back, the only synchronisation of the pass: int64 ``[C, 5]``, or ``[clouds, C, 5]``.  ``scores()`` is
    ``panoptic_scores`` of that.  ``error_flag`` (device int32) collects ``_lib.PANOPTIC_ERR_*`` over the pass; ``check()`` reads it
    back and raises."""

    def __init__(self, num_classes, include=None, things=None, min_points=30, per_cloud=False, device="cuda"):
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Pn2Error("PanopticEvaluator: the HIP device is the only implementation")
        C = self.num_classes
        self.include = torch.ones(C, device=self.device, dtype=torch.int32) if include is None else \
            _class_mask(include, C, self.device, "include")
        self.things = _class_mask(things, C, self.device, "things")
        self.min_points = int(min_points)
        self.per_cloud = bool(per_cloud)
        self.error_flag = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.batches = []                                            # (first slot, slots, rows) per update
        self._tape = torch.zeros(16 if self.per_cloud else 1, C, 5, device=self.device, dtype=torch.int64)
        self._used = 0 if self.per_cloud else 1
        self._work = None

    def _reserve(self, k):
        while self._used + k > self._tape.shape[0]:
            grown = torch.zeros(2 * self._tape.shape[0], self.num_classes, 5, device=self.device, dtype=torch.int64)
            grown[:self._used] = self._tape[:self._used]
            self._tape = grown
        return self._tape[self._used:self._used + k]

    def update(self, pred_sem, pred_inst, gt_sem, gt_inst, row_begin=None, row_count=None, max_rows=None):
        """One batch in any of ``panoptic_counts``' input shapes."""
        if row_begin is not None:
            B, bound = int(row_begin.numel()), int(gt_sem.numel()) if max_rows is None else int(max_rows)
        elif gt_sem.dim() == 2:
            B, bound = int(gt_sem.shape[0]), int(gt_sem.shape[1])
        else:
            B, bound = 1, int(gt_sem.numel())
        need = _lib.workspace_bytes("pn2_panoptic_workspace_bytes", (B, bound), _lib.Pn2Error,
                                    "PanopticEvaluator.update: B = %d, max_rows = %d are not supported" % (B, bound))
        if self._work is None or self._work.numel() < need:
            self._work = panoptic_workspace(B, bound, self.device)
        slot = self._reserve(B) if self.per_cloud else self._tape[0]
        if B > 0:
            panoptic_counts(pred_sem, pred_inst, gt_sem, gt_inst, self.num_classes, self.include, self.things, self.min_points,
                            row_begin, row_count, max_rows, per_cloud=self.per_cloud, out=slot, err=self.error_flag, work=self._work)
        if self.per_cloud:
            self.batches.append((self._used, B, int(gt_sem.numel())))
            self._used += B
        else:
            self.batches.append((0, 1, int(gt_sem.numel())))

    def update_scan(self, scan_labels, scan_instances, gt_words, learning_map, labels_are_raw=True):
        """One scan as ``FrameSegmenter.label_scan(..., instances=)`` leaves it against its ``.label`` file.  ``scan_labels`` /
        ``scan_instances``: the result's entries of those names (``scan_instances`` holds ``id + 1`` and 0 for "none", which becomes
        id -1 here); ``gt_words``: the ground truth's uint32 words (array or 32-bit tensor, ``kitti.split_label_words`` splits them);
        ``learning_map``: int32 DEVICE look-up table raw id -> class of this evaluator, -1 where the map has none (``ScanFilter.lut``).
        Both semantic halves go through it (``labels_are_raw=False``: ``scan_labels`` already holds this evaluator's classes).  A raw
        id outside the table becomes class -1: the row is dropped and ``error_flag`` gets ``PANOPTIC_ERR_CLASS``."""
        from . import kitti
        gt_raw, gt_inst = kitti.split_label_words(gt_words, self.device)
        lut = learning_map.to(device=self.device, dtype=torch.int32)

        def mapped(raw):
            raw = raw.to(torch.int64)
            inside = (raw >= 0) & (raw < lut.numel())
            return torch.where(inside, lut[raw.clamp(0, lut.numel() - 1)], -1).to(torch.int32)

        pred_sem = mapped(scan_labels.reshape(-1)) if labels_are_raw else scan_labels.reshape(-1).to(torch.int32)
        pred_inst = scan_instances.reshape(-1).to(torch.int32) - 1
        if pred_sem.numel() != gt_raw.numel():
            raise ValueError("update_scan: %d predicted rows, %d ground-truth words" % (pred_sem.numel(), gt_raw.numel()))
        self.update(pred_sem, pred_inst, mapped(gt_raw), gt_inst)

    def tables(self):
        t = self._tape[:self._used].cpu().numpy()
        return t if self.per_cloud else t[0]

    def scores(self):
        return panoptic_scores(self.tables(), self.include)

    def check(self):
        """Reads ``error_flag`` back: ``KeyError`` for a ground-truth class outside ``[0, C)``, ``ValueError`` for a cloud whose
        rows left the tensors."""
        flag = int(self.error_flag.item())
        if flag & _lib.PANOPTIC_ERR_CLASS:
            raise KeyError("a ground-truth class lies outside [0, num_classes)")
        if flag & _lib.PANOPTIC_ERR_ROWS:
            raise ValueError("PanopticEvaluator: a cloud's row_begin / row_count leaves the label tensors")
