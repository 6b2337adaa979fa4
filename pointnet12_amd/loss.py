"""The criteria either side of the hot path, on the HIP library.

``nll_loss(log_probs, target)`` is a drop-in for ``torch.nn.functional.nll_loss`` as the reference calls it:
``F.nll_loss(pred, target)`` on ``[B*N, C]`` log-probabilities (semseg.py:143, mean over all points), with an optional
class weight.  ATen's kernel for this reduction runs in a single workgroup (66 us forward + 37 us backward at
65 536 rows, fully exposed between the forward and the backward pass); ``pn2_nll_loss_fwd`` spreads it over the
chip with fp64 partials combined in a fixed order.

``cross_entropy`` / ``CrossEntropyLoss`` are ``torch.nn.functional.cross_entropy`` / ``nn.CrossEntropyLoss`` for
class-index targets: the criterion of the SemanticKITTI loop, ``nn.CrossEntropyLoss()(logits.transpose(2, 1), target)``
(pcdseg.py:178-179: no weight, the input is the model's ``[B, N, C]`` output seen through a class-dim-1 view).  One
launch each way (``pn2_cross_entropy_fwd`` / ``_bwd``), the input read where it lies, 4 bytes per row kept for the backward.

``lovasz_softmax`` / ``LovaszSoftmax`` are the Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018), the surrogate of mean IoU
that SemanticKITTI baselines add to cross-entropy; the reference has none.  One segmented stable radix sort orders every
(image, class) segment at once (``pn2_lovasz_fwd`` / ``_bwd``), with no read-back, so it captures into the step graph.
"""
import torch

from . import _lib

_p = _lib.ptr


class _NllLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target, weight, ignore_index):
        lib, st = _lib.load(), _lib.stream()
        R, C = logp.shape
        from .pointnet_util import _zeros_small                         # the zero arena: no fill launch of its own
        ws = _zeros_small(int(lib.pn2_nll_loss_workspace_bytes(R)), logp.device)
        res = torch.empty(2, device=logp.device, dtype=torch.float32)          # loss, sum of weights
        _lib.check(lib.pn2_nll_loss_fwd(_p(logp), C, _p(target), _p(weight), R, C, ignore_index, _p(ws), res.data_ptr(),
                                        res.data_ptr() + 4, st), "pn2_nll_loss_fwd")
        ctx.save_for_backward(target, weight, res)
        ctx.meta = (R, C, ignore_index)
        return res[0]

    @staticmethod
    def backward(ctx, grad):
        lib, st = _lib.load(), _lib.stream()
        target, weight, res = ctx.saved_tensors
        R, C, ignore_index = ctx.meta
        grad = grad.contiguous().float()
        dlogp = torch.empty(R, C, device=target.device, dtype=torch.float32)
        _lib.check(lib.pn2_nll_loss_bwd(_p(target), _p(weight), R, C, ignore_index, _p(grad), res.data_ptr() + 4, _p(dlogp),
                                        C, st), "pn2_nll_loss_bwd")
        return dlogp, None, None, None


def nll_loss(log_probs, target, weight=None, ignore_index=-100):
    """``F.nll_loss(log_probs, target, weight, ignore_index=ignore_index)`` with reduction "mean".

    log_probs ``[R, C]`` float32 on the GPU (``[B, N, C]`` is flattened as the reference's ``view(-1, C)``
    does), target int64 ``[R]``.  There is no CPU path: tensors must live on the HIP device."""
    if log_probs.dim() > 2:
        log_probs = log_probs.reshape(-1, log_probs.shape[-1])
    if not log_probs.is_cuda:
        raise _lib.Pn2Error("nll_loss: log_probs must be a GPU tensor (the HIP library is the only implementation)")
    if log_probs.dtype != torch.float32:
        raise TypeError("nll_loss: float32 log-probabilities expected, got %s" % log_probs.dtype)
    target = target.reshape(-1)
    if target.dtype != torch.int64:
        target = target.long()
    if target.shape[0] != log_probs.shape[0]:
        raise ValueError("nll_loss: %d rows of log-probabilities, %d targets" % (log_probs.shape[0], target.shape[0]))
    if target.device != log_probs.device:
        target = target.to(log_probs.device)
    if weight is not None:
        weight = weight.to(device=log_probs.device, dtype=torch.float32).contiguous()
        if weight.numel() != log_probs.shape[1]:
            raise ValueError("nll_loss: weight must have one entry per class")
    return _NllLoss.apply(log_probs.contiguous(), target.contiguous(), weight, int(ignore_index))


_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def _ce_layout(x):
    """How ``pn2_cross_entropy_*`` reads ``x`` ([R, C] or [B, C, d1, ...]) in place -> (R, ld, inner), or None.

    Row-major: with the class dim moved last, the classes are adjacent and the leading dims collapse into rows of one pitch
    ld >= C (a contiguous [R, C], a column slice of a padded buffer, the transposed view of a contiguous [B, N, C]).
    Class-strided: contiguous [B, C, N] (a [R, C] whose transpose is contiguous is B = 1)."""
    C = x.shape[1]
    y = x.movedim(1, -1)
    lead = [(n, st) for n, st in zip(y.shape[:-1], y.stride()[:-1]) if n != 1]
    R = 1
    for n, _ in lead:
        R *= n
    if C == 1 or y.stride(-1) == 1:
        ld = lead[-1][1] if lead else C
        if ld >= C and all(a[1] == b[0] * b[1] for a, b in zip(lead[:-1], lead[1:])) and ld < 2 ** 31:
            return R, ld, 0
    if x.dim() == 2:
        x = x.t().unsqueeze(0)
    if x.is_contiguous():
        return R, 0, R // x.shape[0]
    return None


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, weight, ignore_index, reduction, label_smoothing, layout):
        lib, st = _lib.load(), _lib.stream()
        R, ld, inner = layout
        C = x.shape[1]
        lse = torch.empty(R, device=x.device, dtype=torch.float32)       # log sum exp(x - max x) per row
        if reduction == 0:
            out, res, ws = torch.empty(target.shape, device=x.device, dtype=torch.float32), None, None
        else:
            from .pointnet_util import _zeros_small                       # the zero arena: no fill launch of its own
            ws = _zeros_small(int(lib.pn2_cross_entropy_workspace_bytes(R)), x.device)
            res = torch.empty(2, device=x.device, dtype=torch.float32)    # loss, sum of weights
            out = res[0]
        _lib.check(lib.pn2_cross_entropy_fwd(_p(x), ld, inner, _p(target), _p(weight), R, C, ignore_index, label_smoothing,
                                             reduction, _p(ws), _p(lse), out.data_ptr(), None if res is None else res.data_ptr() + 4,
                                             st), "pn2_cross_entropy_fwd")
        ctx.save_for_backward(x, target, weight, lse, res)
        ctx.meta = (R, C, ld, inner, ignore_index, reduction, label_smoothing)
        return out

    @staticmethod
    def backward(ctx, grad):
        lib, st = _lib.load(), _lib.stream()
        x, target, weight, lse, res = ctx.saved_tensors
        R, C, ld, inner, ignore_index, reduction, label_smoothing = ctx.meta
        grad = grad.contiguous().float()                                  # a scalar, or one value per row ("none")
        dx = torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=torch.float32)      # the input's own layout
        _lib.check(lib.pn2_cross_entropy_bwd(_p(x), ld, inner, _p(target), _p(weight), _p(lse), R, C, ignore_index,
                                             label_smoothing, reduction, _p(grad), None if res is None else res.data_ptr() + 4,
                                             _p(dx), st), "pn2_cross_entropy_bwd")
        return dx, None, None, None, None, None, None


def cross_entropy(input, target, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
    """``F.cross_entropy(input, target, weight, ignore_index=, reduction=, label_smoothing=)`` for class-index targets.

    input float32 on the GPU, ``[R, C]`` or ``[B, C, d1, ...]`` (classes in dim 1, C <= 64), read in place: row-major at any
    row pitch, the transposed view of a contiguous ``[B, N, C]`` tensor (pcdseg.py:178) or contiguous ``[B, C, N]``; any
    other layout is refused (no hidden ``.contiguous()``).  target int64 ``[R]`` / ``[B, d1, ...]``.  The gradient comes back
    with the input's strides.  No host synchronisation: forward and backward capture into a graph -- provided target and
    weight already are int64 / float32 tensors on the input's device; otherwise they are converted and copied there on every
    call (as ``nll_loss`` does), and a host-to-device copy does not belong inside a capture."""
    if reduction not in _REDUCTIONS:
        raise ValueError("cross_entropy: %r is not a valid value for reduction" % (reduction,))
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError("cross_entropy: label_smoothing must be between 0.0 and 1.0, got %r" % (label_smoothing,))
    if input.dtype != torch.float32:
        raise TypeError("cross_entropy: float32 logits expected, got %s" % input.dtype)
    if target.is_floating_point():
        raise NotImplementedError("cross_entropy: class-probability targets are not supported, class indices only")
    if input.dim() < 2:
        raise ValueError("cross_entropy: input must be [R, C] or [B, C, d1, ...], got %s" % (tuple(input.shape),))
    if tuple(target.shape) != tuple(input.shape[:1] + input.shape[2:]):
        raise ValueError("cross_entropy: input %s wants a target of shape %s, got %s"
                         % (tuple(input.shape), tuple(input.shape[:1] + input.shape[2:]), tuple(target.shape)))
    C = input.shape[1]
    if weight is not None and weight.numel() != C:
        raise ValueError("cross_entropy: weight must have one entry per class")
    if C > 64:
        raise _lib.Pn2Error("cross_entropy: %d classes, the kernels hold a row of at most 64" % C)
    if input.numel() == 0:
        raise ValueError("cross_entropy: empty input")
    layout = _ce_layout(input)
    if layout is None:
        raise _lib.Pn2Error("cross_entropy: input of shape %s and strides %s is neither row-major rows of classes nor "
                            "contiguous [B, C, N]; lay it out as one of the two" % (tuple(input.shape), input.stride()))
    if not input.is_cuda:
        raise _lib.Pn2Error("cross_entropy: input must be a GPU tensor (the HIP library is the only implementation)")
    target = target.to(device=input.device, dtype=torch.int64).contiguous()
    if weight is not None:
        weight = weight.to(device=input.device, dtype=torch.float32).contiguous()
    return _CrossEntropy.apply(input, target, weight, int(ignore_index), _REDUCTIONS[reduction], float(label_smoothing), layout)


class CrossEntropyLoss(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss`` on :func:`cross_entropy` (``size_average`` / ``reduce`` are torch's deprecated spellings
    of ``reduction`` and are mapped the way torch maps them).  ``weight`` is a buffer: move the module to the device
    (``.to(device)``) like any other, or every call copies the weight there."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        super().__init__()
        if size_average is not None or reduce is not None:
            reduction = torch.nn._reduction.legacy_get_string(size_average, reduce)
        self.register_buffer("weight", weight)
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing

    def forward(self, input, target):
        return cross_entropy(input, target, self.weight, self.ignore_index, self.reduction, self.label_smoothing)


# ------------------------------------------------------------------------------------------------------------ Lovasz-Softmax
_lovasz_ws = {}          # (device, stream, bytes) -> the sort's workspace: it holds nothing between calls, one per shape is enough


def _lovasz_workspace(nbytes, device):
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, device=device, dtype=torch.uint8)      # the graph's own pool keeps it alive with the graph
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, nbytes)
    ws = _lovasz_ws.get(key)
    if ws is None:
        ws = _lovasz_ws[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return ws


class _LovaszSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, class_mask, present_only, images, ignore_index, from_logits, layout):
        lib, st = _lib.load(), _lib.stream()
        R, ld, inner = layout
        C = x.shape[1]
        nbytes = _lib.workspace_bytes("pn2_lovasz_workspace_bytes", (R, C, images), _lib.Pn2Error,
                                      "lovasz_softmax: %d rows of %d classes in %d images are beyond the kernels' index range" % (R, C, images))
        ws = _lovasz_workspace(nbytes, x.device)
        dp = torch.empty(R, C, device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        _lib.check(lib.pn2_lovasz_fwd(_p(x), ld, inner, _p(target), R, C, images, ignore_index, int(from_logits), _p(class_mask),
                                      int(present_only), _p(ws), _p(dp), None, _p(loss), st), "pn2_lovasz_fwd")
        ctx.save_for_backward(x, dp)
        ctx.meta = (R, C, ld, inner, int(from_logits))
        return loss

    @staticmethod
    def backward(ctx, grad):
        lib, st = _lib.load(), _lib.stream()
        x, dp = ctx.saved_tensors
        R, C, ld, inner, from_logits = ctx.meta
        grad = grad.contiguous().float()
        dx = torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=torch.float32)      # the input's own layout
        _lib.check(lib.pn2_lovasz_bwd(_p(x), ld, inner, _p(dp), R, C, from_logits, _p(grad), _p(dx), st), "pn2_lovasz_bwd")
        return dx, None, None, None, None, None, None, None


_lovasz_masks = {}       # (device, C, classes) -> int32[C] on the device: a list of classes is copied there once


def lovasz_softmax(input, target, classes="present", per_image=False, ignore_index=-100, from_logits=True):
    """The Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018), the surrogate that optimises mean IoU; the rule is stated in
    include/pn2.h (``pn2_lovasz_fwd``) and in numpy in tests/lovasz_ref.py.

    input float32 on the GPU, ``[R, C]`` or ``[B, C, d1, ...]`` (classes in dim 1, C <= 64) in the layouts :func:`cross_entropy`
    reads in place; logits or log-probabilities with ``from_logits`` (the softmax is part of the kernel), probabilities without.
    target int64 ``[R]`` / ``[B, d1, ...]``; rows equal to ``ignore_index`` take no part.  ``classes``: "present" (classes with at
    least one target row), "all", or a list of class ids.  ``per_image`` (``[B, C, ...]`` inputs only): the loss of every image,
    then the mean over all B.  One segmented stable radix sort serves every class at once; nothing is read back to the host, so
    forward and backward capture into a graph when target already is an int64 tensor on the input's device (a list of classes is
    uploaded once, by the first call that names it: make that call before the capture, as a warm-up step does).  The gradient
    comes back with the input's strides."""
    if input.dtype != torch.float32:
        raise TypeError("lovasz_softmax: float32 input expected, got %s" % input.dtype)
    if target.is_floating_point():
        raise NotImplementedError("lovasz_softmax: class-probability targets are not supported, class indices only")
    if input.dim() < 2:
        raise ValueError("lovasz_softmax: input must be [R, C] or [B, C, d1, ...], got %s" % (tuple(input.shape),))
    if tuple(target.shape) != tuple(input.shape[:1] + input.shape[2:]):
        raise ValueError("lovasz_softmax: input %s wants a target of shape %s, got %s"
                         % (tuple(input.shape), tuple(input.shape[:1] + input.shape[2:]), tuple(target.shape)))
    C = input.shape[1]
    if C > 64:
        raise _lib.Pn2Error("lovasz_softmax: %d classes, the kernels hold a row of at most 64" % C)
    if input.numel() == 0:
        raise ValueError("lovasz_softmax: empty input")
    if per_image and input.dim() < 3:
        raise _lib.Pn2Error("lovasz_softmax: per_image needs a [B, C, d1, ...] input, got %s" % (tuple(input.shape),))
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError("lovasz_softmax: classes must be 'present', 'all' or a list of class ids, got %r" % (classes,))
        ids = None
    else:
        ids = tuple(sorted(set(int(c) for c in classes)))
        if any(c < 0 or c >= C for c in ids):
            raise ValueError("lovasz_softmax: class ids %r outside [0, %d)" % (ids, C))
    layout = _ce_layout(input)
    if layout is None:
        raise _lib.Pn2Error("lovasz_softmax: input of shape %s and strides %s is neither row-major rows of classes nor "
                            "contiguous [B, C, N]; lay it out as one of the two" % (tuple(input.shape), input.stride()))
    if not input.is_cuda:
        raise _lib.Pn2Error("lovasz_softmax: input must be a GPU tensor (the HIP library is the only implementation)")
    images = input.shape[0] if per_image else 1
    if images > 1 and layout[2] not in (0, layout[0] // images):
        raise _lib.Pn2Error("lovasz_softmax: per_image cannot read a transposed [R, C] as images")
    target = target.to(device=input.device, dtype=torch.int64).contiguous()
    mask = None
    if ids is not None:
        key = (input.device.index, C, ids)
        mask = _lovasz_masks.get(key)
        if mask is None:
            m = torch.zeros(C, dtype=torch.int32)
            m[list(ids)] = 1
            mask = _lovasz_masks[key] = m.to(input.device)
    return _LovaszSoftmax.apply(input, target, mask, classes == "present", images, int(ignore_index), bool(from_logits), layout)


class LovaszSoftmax(torch.nn.Module):
    """:func:`lovasz_softmax` as a module, with the same arguments."""

    def __init__(self, classes="present", per_image=False, ignore_index=-100, from_logits=True):
        super().__init__()
        self.classes = classes
        self.per_image = per_image
        self.ignore_index = ignore_index
        self.from_logits = from_logits

    def forward(self, input, target):
        return lovasz_softmax(input, target, self.classes, self.per_image, self.ignore_index, self.from_logits)
