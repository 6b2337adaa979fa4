"""One Adam update (torch/optim/adam.py::_single_tensor_adam, the expressions of ``adam_elem`` in csrc/train.hip) stated three ways.

``scalars``    the seven fp32 scalars ``adam_scalars`` (train.hip) forms from Python doubles, returned as the exact doubles those fp32
               values are, so that the rounding of a scalar is no part of any error below.  ``nudge=(i, j)`` moves ``step_size`` and
               ``bc2_sqrt`` by i and j fp32 ulps: the two scalars that come out of a ``pow`` in fp64, the only operation whose device
               and host results may differ, and only by enough to move one fp32 rounding.
``adam_ref``   the fp64 values p', m', v' of the same expressions (both lerp forms) and a per-element FIRST-ORDER bound E_p, E_m, E_v on
               what a correct fp32 evaluation may differ from them by.  The rule: every fp32 operation contributes 2^-24 of the
               magnitude of its (fp64) result -- half an ulp is at most that -- and a contribution reaches the outputs multiplied by the
               absolute derivatives of the operations after it.  A sum that cancels (g + wd*p, g - m, m + w*d) therefore carries the
               errors of its OPERANDS whatever its result is; 2^-149 is added so that an exact zero has a bound.  Two operations add
               nothing because they are exact in fp32: 1 - w for w in [0.5, 1] (Sterbenz) and x + eps for eps == 0.
               The assertion on any fp32 evaluation is |got - ref| <= 2 E elementwise, the 2 covering the second-order terms.
``adam_f32``   the fp32 statement, operation for operation ``oracle/train_ref.adam_step`` (tests/test_adam_ref_cpu.py holds the two to
               equal bits), but taking the scalars: the yardstick for a launch whose device-side ``pow`` moved a scalar by an ulp.

``make_inputs`` draws the operand families and ``HYPER_SETS`` lists the hyper-parameters every Adam test here sweeps.
"""
import math
from collections import namedtuple

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                      # half an fp32 ulp relative to the binade: <= 2^-24 |x|
FLOOR = 2.0 ** -149                 # the smallest fp32 denormal

Scalars = namedtuple("Scalars", "step_size bc2_sqrt beta1_w beta2 one_m_beta2 eps wd")

# (lr, betas, eps, weight_decay, t)
HYPER_SETS = [
    (1e-3, (0.9, 0.999), 1e-8, 0.0, 1),
    (2e-3, (0.9, 0.999), 1e-8, 1e-4, 7),
    (1e-3, (0.9, 0.999), 1e-8, 1e-4, 100000),
    (1e-2, (0.3, 0.5), 1e-3, 1e-2, 3),              # beta1_w = 0.7: the `weight >= 0.5` form of the lerp
    (1e-3, (0.5, 0.999), 1e-8, 0.5, 2),             # beta1_w exactly 0.5: the boundary, which takes that form too
    (1e-3, (0.0, 0.0), 0.0, 0.0, 1),
    (0.0, (0.9, 0.999), 1e-8, 1e-4, 5),             # lr = 0: p keeps its bits while m and v move
]
HYPER_IDS = ["lr%g-b%g,%g-eps%g-wd%g-t%d" % (lr, b[0], b[1], eps, wd, t) for lr, b, eps, wd, t in HYPER_SETS]
NUDGES = [(0, 0)] + [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]


def _ulps(x, k):
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf), dtype=f32)
    return x


def scalars(lr, betas, eps, wd, t, nudge=(0, 0)):
    """adam_scalars of train.hip: Python doubles, rounded to fp32 where a float kernel takes them; returned as exact doubles."""
    beta1, beta2 = betas
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    return Scalars(*(float(x) for x in (_ulps(lr / bc1, nudge[0]), _ulps(math.sqrt(bc2), nudge[1]), f32(1.0 - beta1), f32(beta2),
                                        f32(1.0 - beta2), f32(eps), f32(wd))))


def adam_ref(p, g, m, v, s):
    """fp32 arrays and a ``Scalars`` -> ((p', m', v') in fp64, (E_p, E_m, E_v)).  Nothing is updated in place."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == f32
    p, g, m, v = (x.astype(f64) for x in (p, g, m, v))
    A = np.abs
    if s.wd != 0:
        a = s.wd * p                                            # exact in fp64: two 24-bit significands
        g1 = g + a
        Eg = U * A(a) + U * A(g1)                               # the product's rounding passes the add unchanged, the add's is on top
    else:
        g1, Eg = g, 0.0
    d = g1 - m
    Ed_own = U * A(d)
    w = s.beta1_w
    if w < 0.5:                                                 # m + w * d
        t1 = w * d
        m1 = m + t1
        Em = w * (Eg + Ed_own) + U * A(t1) + U * A(m1)
    else:                                                       # g1 - d * (1 - w); 1 - w is exact, and dm'/dg1 = 1 - (1 - w) = w
        c = 1.0 - w
        assert float(f32(c)) == c
        t1 = d * c
        m1 = g1 - t1
        Em = w * Eg + c * Ed_own + U * A(t1) + U * A(m1)
    q = v * s.beta2
    r = s.one_m_beta2 * g1
    sq_g = r * g1
    v1 = q + sq_g
    Er = s.one_m_beta2 * Eg + U * A(r)
    Ev = U * A(q) + (A(g1) * Er + A(r) * Eg + U * A(sq_g)) + U * A(v1)
    root = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        Eroot = np.where(root > 0, (Ev + FLOOR) / (2 * root), np.sqrt(Ev + FLOOR)) + U * root
        quo = root / s.bc2_sqrt
        Equo = Eroot / s.bc2_sqrt + U * quo
        den = quo + s.eps
        Eden = Equo + (U * den if s.eps != 0 else 0.0)
        ratio = m1 / den
        Eratio = (Em + FLOOR) / den + A(ratio) * Eden / den + U * A(ratio)
        z = s.step_size * ratio
        p1 = p - z
        Ep = s.step_size * Eratio + U * A(z) + U * A(p1)
    return (p1, m1, v1), (Ep + FLOOR, Em + FLOOR, Ev + FLOOR)


def adam_f32(p, g, m, v, s, low_form=None):
    """The fp32 statement on given scalars: every operation one correctly rounded fp32 operation, none fused.  Returns new
    (p', m', v').  ``low_form`` forces one of the lerp's two forms (None: ATen's choice, by the weight)."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == f32
    ss, bc, w, b2, omb2, eps, wd = (f32(x) for x in s)
    if wd != 0:
        g = g + wd * p
    d = g - m
    m1 = m + w * d if (w < 0.5 if low_form is None else low_form) else g - d * (f32(1) - w)
    v1 = v * b2 + omb2 * g * g
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.sqrt(v1) / bc + eps
        p1 = p - ss * (m1 / den)
    return p1, m1, v1


def worst_ratio(got, ref, E):
    """max over elements of |got - ref| / (2 E): the assertion is that it is <= 1."""
    return float((np.abs(got.astype(f64) - ref) / (2 * E)).max())


def cancel_mask(n):
    """The stride whose gradient cancels the weight decay (where it is not one of the every-7th zeros)."""
    i = np.arange(n)
    return (i % 17 == 2) & (i % 7 != 0)


def make_inputs(n, hyper, seed):
    """The operand families of the Adam tests, mixed within one buffer.  Returns fp32 (p, g, m, v) and the index array of the
    planted group (g = m = v = 0 where eps > 0; p = +-0 there when there is weight decay), whose p must keep its bits.

    p ~ randn with some +0, some -0 and some of magnitude 1e4;  g ~ randn * 10^k, k per ELEMENT from -12 .. 2, |g| >= 1e-12 or exactly
    0 (every 7th, unless eps == 0) so that no intermediate is denormal;  with weight decay a stride of g = -(fp32(wd) * p), which the
    weight-decay add cancels;  m = v = 0 at t = 1, else m of the gradient's scale and v of its square (|v| >= 1e-6 * 10^2k) -- on the
    cancelling stride too, where that scale is |wd p|: moments far below the rounding of wd * p would make m' and the denominator
    nothing but rounding error, which no first-order bound describes."""
    lr, betas, eps, wd, t = hyper
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    p = rng.standard_normal(n).astype(f32)
    big = i % 13 == 1
    p[big] = (np.sign(p[big]) * 1e4 * (1 + 0.25 * rng.random(int(big.sum())))).astype(f32)
    p[i % 11 == 3] = f32(0.0)
    p[i % 11 == 5] = f32(-0.0)
    scale = 10.0 ** rng.integers(-12, 3, n)
    g = rng.standard_normal(n) * scale
    g = (np.where(g < 0, -1.0, 1.0) * np.maximum(np.abs(g), 1e-12)).astype(f32)
    if eps != 0:
        g[i % 7 == 0] = 0
    if wd != 0:
        c = cancel_mask(n)
        g[c] = -(f32(wd) * p[c])
        scale[c] = np.abs(g[c])                                     # "the gradient's scale" there is the scale of wd * p
    if t > 1:
        m = (rng.standard_normal(n) * scale).astype(f32)
        v = ((np.maximum(np.abs(rng.standard_normal(n)), 1e-3) * scale) ** 2).astype(f32)
    else:
        m, v = np.zeros(n, f32), np.zeros(n, f32)
    plant = i[i % 19 == 4] if eps != 0 else i[:0]
    g[plant] = 0
    m[plant] = 0
    v[plant] = 0
    if wd != 0:
        p[plant] = np.where(plant % 2 == 0, f32(0.0), f32(-0.0))
    return p, g, m, v, plant
