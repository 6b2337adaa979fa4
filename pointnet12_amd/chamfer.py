"""MI355X-native counterpart of the reference's ``model/chamfer.py``.

Same names, argument order and return type: ``chamfer_batch(p1 [B,N,D], p2 [B,M,D])`` is a 0-dim float32 tensor on the
inputs' device,

    (1/B) * sum_b sum_n min_m || p1[b,n,:] - p2[b,m,:] ||_2

-- ONE direction (p1 -> p2) and the distance, not its square, exactly as the reference defines it.  The reference
repeats both sets to ``[B,N,M,D]``; here the search is ``pn2_chamfer_nn`` (csrc/chamfer.hip), which keeps the running
minimum in registers and writes nothing of size ``N x M``, forward or backward.

Differences from the reference, all deliberate:
  * float32 on the GPU only (the reference takes any floating dtype on any device): another dtype raises
    ``RuntimeError``, a CPU tensor ``Pn2Error``, ``D > 16`` ``Pn2Error`` -- there is no fallback path;
  * ties go to the lowest candidate index, decided on the fp32 squared distance in difference form (the reference's
    ``min`` over fp32 norms does the same on the data it was probed with);
  * non-finite coordinates: a squared distance that is NaN or +inf never wins the search's strict ``<``, so a candidate
    with a NaN or infinite coordinate is never chosen and a query with one gets index 0 and distance +inf -- the value
    becomes +inf where the reference's ``min`` hands a NaN on; no other point's result changes (include/pn2.h);
  * ``nearest_neighbor`` and ``chamfer_symmetric`` are additions.
"""
import torch

from . import _lib
from ._lib import check as _check, ptr as _p
from .pointnet_util import _gpu_f32, _zeros_f32

MAX_D = 16          # include/pn2.h: pn2_chamfer_nn answers PN2_EUNSUPPORTED above


def num(x):
    return x.detach().cpu().numpy()


def _search(p1, p2, want_sum):
    """Contiguous float32 GPU tensors [B,N,D], [B,M,D] -> dist [B,N], idx [B,N], value (0-dim, or None)."""
    lib = _lib.load()
    B, N, D = p1.shape
    M = p2.shape[1]
    dist = torch.empty(B, N, device=p1.device, dtype=torch.float32)
    idx = torch.empty(B, N, device=p1.device, dtype=torch.int64)
    value = torch.empty((), device=p1.device, dtype=torch.float32) if want_sum else None
    ws = torch.empty(int(lib.pn2_chamfer_nn_workspace_bytes(B, N, M, D)), device=p1.device, dtype=torch.uint8)
    _check(lib.pn2_chamfer_nn(_p(p1), _p(p2), B, N, M, D, _p(dist), _p(idx), _p(value), _p(ws), _lib.stream()), "pn2_chamfer_nn")
    return dist, idx, value


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2):
        dist, idx, value = _search(p1, p2, True)
        ctx.save_for_backward(p1, p2, dist, idx)
        return value

    @staticmethod
    def backward(ctx, grad):
        p1, p2, dist, idx = ctx.saved_tensors
        B, N, D = p1.shape
        M = p2.shape[1]
        grad = _gpu_f32(grad, "grad")                        # read on the device: no .item(), the call can be captured
        dp1 = torch.empty_like(p1) if ctx.needs_input_grad[0] else None
        dp2 = _zeros_f32((B, M, D), p1.device) if ctx.needs_input_grad[1] else None
        _check(_lib.load().pn2_chamfer_bwd(_p(p1), _p(p2), _p(dist), _p(idx), _p(grad), B, N, M, D, _p(dp1), _p(dp2),
                                           _lib.stream()), "pn2_chamfer_bwd")
        return dp1, dp2


def _prepare(p1, p2):
    """The reference's own checks first (they need no device), then this package's."""
    assert p1.size(0) == p2.size(0) and p1.size(2) == p2.size(2)
    if p2.size(1) == 0:
        raise IndexError("min(): Expected reduction dim 2 to have non-zero size.")       # what the reference's min() raises
    p1, p2 = _gpu_f32(p1, "p1"), _gpu_f32(p2, "p2")
    if p1.device != p2.device:
        raise _lib.Pn2Error("p1 and p2 must live on the same device")
    if not 1 <= p1.size(2) <= MAX_D:
        raise _lib.Pn2Error("chamfer: point dimension D = %d is not supported (1 <= D <= %d; there is no fallback path)"
                            % (p1.size(2), MAX_D))
    return p1, p2


def chamfer_batch(p1, p2):
    """p1 [B,N,D], p2 [B,M,D] -> the mean over the batch of sum_n min_m ||p1[b,n] - p2[b,m]||  (model/chamfer.py:32-53)."""
    p1, p2 = _prepare(p1, p2)
    if p1.size(0) == 0:
        return torch.full((), float("nan"), device=p1.device, dtype=torch.float32)        # the reference's 0 / 0
    if p1.size(1) == 0:
        return torch.zeros((), device=p1.device, dtype=torch.float32)
    return _Chamfer.apply(p1, p2)


def chamfer_non_batch(p1, p2):
    """p1 [1,N,D], p2 [1,M,D] -> sum_n min_m ||p1[0,n] - p2[0,m]||  (model/chamfer.py:7-30)."""
    assert p1.size(0) == 1 and p2.size(0) == 1
    assert p1.size(2) == p2.size(2)
    return chamfer_batch(p1, p2)


def chamfer_symmetric(p1, p2):
    """``chamfer_batch(p1, p2) + chamfer_batch(p2, p1)``: the two-sided form usually meant by the name."""
    return chamfer_batch(p1, p2) + chamfer_batch(p2, p1)


def nearest_neighbor(p1, p2):
    """For every point of p1 [B,N,D] its nearest point of p2 [B,M,D]: ``(dist [B,N] float32, idx [B,N] int64)``, the lowest
    index on equal distance.  Neither output carries a gradient (``chamfer_batch`` is the differentiable form)."""
    p1, p2 = _prepare(p1.detach(), p2.detach())
    if p1.size(0) == 0 or p1.size(1) == 0:
        return (torch.empty(p1.shape[:2], device=p1.device, dtype=torch.float32),
                torch.empty(p1.shape[:2], device=p1.device, dtype=torch.int64))
    dist, idx, _ = _search(p1, p2, False)
    return dist, idx
