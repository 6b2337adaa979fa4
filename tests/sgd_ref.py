"""torch/optim/sgd.py::_single_tensor_sgd restated in numpy: the arithmetic pn2_sgd_step must have (include/pn2.h).

``sgd_step`` is the fp32 statement.  The four scalars are Python doubles rounded to fp32 once; every ``add(alpha=)`` is ONE
rounding of ``a + alpha*b``, written ``float32(float64(a) + float64(alpha) * float64(b))``: the product of two fp32 numbers is
exact in fp64 (24 + 24 significant bits), so only the sum is rounded before the result goes to fp32, as in a fused
multiply-add (tests/test_sgd_cpu.py holds this form to ATen bit for bit).  The ``mul_`` of the buffer is rounded on its own.

``sgd_step64`` evaluates the same updates in fp64 (scalars un-rounded): the yardstick for an fp32 evaluation's own error.

Both update ``p`` (and ``buf``) in place and return the buffer (None without momentum).  ``t`` is the step number, from 1.
"""
import numpy as np

f32, f64 = np.float32, np.float64


def _fma(alpha, b, a):
    """float32(a + alpha*b) with one rounding; alpha an fp32 scalar, a and b fp32 arrays."""
    return (a.astype(f64) + f64(alpha) * b.astype(f64)).astype(f32)


def sgd_step(p, grad, buf, t, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    assert p.dtype == f32 and grad.dtype == f32 and (buf is None or buf.dtype == f32)
    wd, om, mu, nl = f32(weight_decay), f32(1.0 - dampening), f32(momentum), f32(-lr)
    g = -grad if maximize else grad
    if weight_decay != 0:
        g = _fma(wd, p, g)                                   # grad.add(param, alpha=weight_decay)
    if momentum != 0:
        if t == 1:
            buf = g.copy() if buf is None else buf
            buf[...] = g                                     # buf = clone(grad): no dampening on the first step
        else:
            buf[...] = _fma(om, g, buf * mu)                 # buf.mul_(momentum) rounded, then .add_(grad, alpha=1-dampening)
        g = _fma(mu, buf, g) if nesterov else buf
    p[...] = _fma(nl, g, p)                                  # param.add_(grad, alpha=-lr)
    return buf if momentum != 0 else None


def sgd_step64(p, grad, buf, t, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    assert p.dtype == f64 and (buf is None or buf.dtype == f64)
    g = grad.astype(f64)
    g = -g if maximize else g
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        if t == 1:
            buf = g.copy() if buf is None else buf
            buf[...] = g
        else:
            buf[...] = buf * momentum + (1.0 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    p[...] = p - lr * g
    return buf if momentum != 0 else None


# the option sets every SGD test sweeps: weight decay 0 / 1e-4, momentum 0 / 0.5 / 0.9, dampening 0 / 0.1 / 0.25, nesterov on / off,
# and maximize
OPTION_SETS = [
    dict(),
    dict(weight_decay=1e-4),
    dict(momentum=0.9),
    dict(momentum=0.9, weight_decay=1e-4, nesterov=True),
    dict(momentum=0.5, dampening=0.1),
    dict(momentum=0.9, dampening=0.25, weight_decay=1e-4),
    dict(momentum=0.9, weight_decay=1e-4, maximize=True),
]
