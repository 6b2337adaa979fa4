"""GPU: pn2_adam_step at the C ABI -- raw pointers, outputs read back, state carried on the device and in the reference from launch to
launch -- held element by element to ``oracle/train_ref.adam_step`` (bits) and to the fp64 rule of tests/adam_ref.py (within 2 E).

Acceptance of every accepted launch (``check``):
  * m' and v' EQUAL the oracle's bits: they depend on no scalar the device forms with pow, and train.hip is built with
    -ffp-contract=off and correctly rounded fp32 divide and square root, so both sides run the same separately rounded operations;
  * p' EQUALS the oracle's bits for ONE of the nine (step_size, bc2_sqrt) candidates, each moved by -1, 0 or +1 fp32 ulp, the same
    one for every element of the launch: only the device's fp64 pow may differ from the host's, and only by enough to move one
    fp32 rounding.  At t = 1 (pow(beta, 1) = beta) it must be the un-nudged one.  The matched candidate is printed;
  * p', m', v' lie within 2 E of adam_ref on the matched candidate's scalars; the worst |err| / (2 E) is printed.
Every buffer sits between guard elements, which must come back unchanged.

Measured on an MI355X, after the checks were written: every launch of this file (55) matched the un-nudged candidate, so param,
exp_avg and exp_avg_sq were bit-equal to the oracle throughout; worst |err| / (2 E) 0.499 (p), 0.494 (m), 0.495 (v)."""
import numpy as np
import pytest
import torch

import adam_ref as R
from oracle import train_ref as TR
from pointnet12_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 4                                   # floats in front of an aligned range (16 bytes) and at least that many behind
SENTINEL = (11.0, 22.0, 33.0, 44.0)         # per buffer: p, g, m, v
N_VEC_STRIDE = 8192 * 256 * 4 + 5           # more float4s than 8 192 workgroups x 256 threads cover in one trip, + a 1-element tail
N_SCALAR_STRIDE = 8192 * 256 + 3            # the same for the scalar kernel
SIZES = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 4099]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


class Slab:
    """Four guarded device buffers p, g, m, v of n floats; ``off[i]`` = 1 puts buffer i one float off a 16-byte boundary."""

    def __init__(self, dev, n, off=(0, 0, 0, 0)):
        self.n, self.off = n, off
        self.hold = [torch.full((n + 2 * GUARD + 1,), s, device=dev) for s in SENTINEL]
        self.view = [h[GUARD + o:GUARD + o + n] for h, o in zip(self.hold, off)]
        for h, x, o in zip(self.hold, self.view, off):
            assert h.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4 * o
        self.ptrs = tuple(x.data_ptr() for x in self.view)

    def put(self, p=None, g=None, m=None, v=None):
        for x, a in zip(self.view, (p, g, m, v)):
            if a is not None:
                x.copy_(torch.from_numpy(a))

    def get(self):
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy().copy() for x in self.view)

    def guards_intact(self):
        for h, s, o in zip(self.hold, SENTINEL, self.off):
            h = h.cpu().numpy()
            assert (h[:GUARD + o] == s).all() and (h[GUARD + o + self.n:] == s).all(), "a guard element was written"


def step(lib, slab, hyper, zero_grad=0, lr_dev=None, step_dev=None, host_lr=None, host_step=None):
    lr, (b1, b2), eps, wd, t = hyper
    return lib.pn2_adam_step(*slab.ptrs, slab.n, lr if host_lr is None else host_lr, b1, b2, eps, wd,
                             t if host_step is None else host_step, _lib.ptr(lr_dev), _lib.ptr(step_dev), zero_grad, _lib.stream())


def oracle(p, g, m, v, hyper):
    lr, betas, eps, wd, t = hyper
    p, m, v = p.copy(), m.copy(), v.copy()
    TR.adam_step(p, g.copy(), m, v, t, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    return p, m, v


def check(tag, got, before, hyper, plant=None):
    """The acceptance of the module docstring for one launch: ``got`` = (p', g, m', v') read back, ``before`` = (p, g, m, v)."""
    p0, g0, m0, v0 = before
    want = oracle(p0, g0, m0, v0, hyper)
    for k, what in ((1, "exp_avg"), (2, "exp_avg_sq")):
        differ = bits(got[k + 1]) != bits(want[k])
        assert not differ.any(), "%s: %s differs from the oracle's bits on %d of %d elements, first at %d" % (
            tag, what, int(differ.sum()), differ.size, int(np.argmax(differ)))
    nudge = None
    if (bits(got[0]) == bits(want[0])).all():
        nudge = (0, 0)
    else:                                               # the other eight only when the un-nudged one does not match
        for cand in R.NUDGES[1:]:
            if (bits(R.adam_f32(p0, g0, m0, v0, R.scalars(*hyper, nudge=cand))[0]) == bits(got[0])).all():
                nudge = cand
                break
    differ = bits(got[0]) != bits(want[0])
    assert nudge is not None, "%s: param matches the oracle's bits for none of the nine scalar candidates; against the un-nudged one " \
        "%d of %d elements differ, first at %d" % (tag, int(differ.sum()), differ.size, int(np.argmax(differ)))
    assert nudge == (0, 0) or hyper[4] != 1, "%s: a nudged candidate %s at t = 1" % (tag, nudge)
    ref, E = R.adam_ref(p0, g0, m0, v0, R.scalars(*hyper, nudge=nudge))
    ratios = [R.worst_ratio(a, b, e) for a, b, e in zip((got[0], got[2], got[3]), ref, E)]
    print("adam %-34s n %-8d %-38s candidate (step_size %+d ulp, bc2_sqrt %+d ulp)  worst |err|/(2E): p %.3f  m %.3f  v %.3f" % (
        tag, p0.size, hyper, nudge[0], nudge[1], *ratios))
    assert max(ratios) <= 1.0, (tag, ratios)
    if plant is not None and plant.size:
        assert (bits(got[0])[plant] == bits(p0)[plant]).all(), "%s: p moved where g = m = v = 0" % tag
    if hyper[0] == 0:                                   # lr = 0: p keeps its bits (but -0 - (-0) = +0, as in ATen) while m and v move
        assert (got[0] == p0).all() and (bits(got[0]) == bits(p0))[bits(p0) != 0x80000000].all()
        assert p0.size < 8 or ((bits(got[2]) != bits(m0)).any() and (bits(got[3]) != bits(v0)).any())
    return nudge


def next_grad(g, p, hyper):
    """A second gradient from the first: rolled by one element and scaled by -1/2 (exact), its cancelling stride following p."""
    g = np.roll(g, 1) * np.float32(-0.5)
    if hyper[3] != 0:
        c = R.cancel_mask(g.size)
        g[c] = -(np.float32(hyper[3]) * p[c])
    return g


def run_one(dev, n, hyper, off=(0, 0, 0, 0), seed=0, zero_grad=0, tag=""):
    lib = _lib.load()
    p, g, m, v, plant = R.make_inputs(n, hyper, seed)
    slab = Slab(dev, n, off)
    slab.put(p, g, m, v)
    assert step(lib, slab, hyper, zero_grad) == 0
    got = slab.get()
    slab.guards_intact()
    check(tag, got, (p, g, m, v), hyper, plant)
    return got, (p, g, m, v)


# ------------------------------------------------------------------------------------------------ 1. the vector kernel, every tail
@pytest.mark.parametrize("k", range(len(R.HYPER_SETS)), ids=R.HYPER_IDS)
def test_adam_step_every_hyper_set(dev, k):
    """n = 4099: 1 024 float4s over four workgroups and a 3-element tail; every family in one buffer."""
    got, before = run_one(dev, 4099, R.HYPER_SETS[k], seed=10 + k, tag="aligned")
    assert (bits(got[1]) == bits(before[1])).all()                  # zero_grad == 0 leaves the gradient


@pytest.mark.parametrize("k", [1, 3], ids=[R.HYPER_IDS[1], R.HYPER_IDS[3]])
@pytest.mark.parametrize("n", SIZES[:-1])
def test_adam_step_sizes_and_tails(dev, n, k):
    """Tail lengths 0 .. 3 at one float4, around one workgroup and around four; n < 4: the vector loop is empty."""
    run_one(dev, n, R.HYPER_SETS[k], seed=100 * k + n, tag="aligned")


# ------------------------------------------------------------------------------------------------ 2. the scalar kernel
@pytest.mark.parametrize("k", [1, 3], ids=[R.HYPER_IDS[1], R.HYPER_IDS[3]])
def test_adam_step_unaligned_pointers_select_the_scalar_kernel(dev, k):
    """All four pointers one float off a 16-byte boundary, then each one alone: any one makes the launcher take the scalar kernel, and
    every such run gives the bits of the aligned run."""
    hyper, n = R.HYPER_SETS[k], 1030
    aligned, _ = run_one(dev, n, hyper, seed=50 + k, tag="aligned")
    for off in ((1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        got, _ = run_one(dev, n, hyper, off, seed=50 + k, tag="unaligned %s" % (off,))
        for a, b, what in zip(got, aligned, ("param", "grad", "exp_avg", "exp_avg_sq")):
            assert (bits(a) == bits(b)).all(), (off, what)


# ------------------------------------------------------------------------------------------------ 3. the grid-stride loops
def two_chained_steps(dev, n, off, hyper, seed, tag):
    lib = _lib.load()
    p, g, m, v, plant = R.make_inputs(n, hyper, seed)
    slab = Slab(dev, n, off)
    slab.put(p, g, m, v)
    for i in range(2):
        h = hyper[:4] + (hyper[4] + i,)
        assert step(lib, slab, h) == 0
        got = slab.get()
        check("%s step %d" % (tag, i + 1), got, (p, g, m, v), h, plant if i == 0 else None)
        assert (bits(got[1]) == bits(g)).all()
        p, m, v = got[0], got[2], got[3]                            # the device's state is the reference's from here on
        if i == 0:
            g = next_grad(g, p, hyper)
            slab.put(g=g)
    slab.guards_intact()


def test_adam_step_vector_grid_stride_loop(dev):
    """8 192 workgroups, the float4 loop takes a second trip, a 1-element tail after the last whole float4."""
    two_chained_steps(dev, N_VEC_STRIDE, (0, 0, 0, 0), R.HYPER_SETS[1], 7, "vector grid stride")


def test_adam_step_scalar_grid_stride_loop(dev):
    """Unaligned: 8 192 workgroups of the scalar kernel, whose loop takes a second trip for 3 elements."""
    two_chained_steps(dev, N_SCALAR_STRIDE, (1, 1, 1, 1), R.HYPER_SETS[1], 8, "scalar grid stride")


# ------------------------------------------------------------------------------------------------ 4. zero_grad
@pytest.mark.parametrize("off", [(0, 0, 0, 0), (1, 1, 1, 1)], ids=["vector", "scalar"])
@pytest.mark.parametrize("n", [7, 1030])
def test_adam_step_zero_grad(dev, n, off):
    hyper = R.HYPER_SETS[1]
    kept, before = run_one(dev, n, hyper, off, seed=70 + n, zero_grad=0, tag="zero_grad=0")
    assert (bits(kept[1]) == bits(before[1])).all() and before[1].any()
    # zero_grad = 1: the same update, exactly the range cleared (tail included, +0 bits), the guards intact
    lib = _lib.load()
    slab = Slab(dev, n, off)
    slab.put(*before)
    assert step(lib, slab, hyper, zero_grad=1) == 0
    got = slab.get()
    slab.guards_intact()
    assert not bits(got[1]).any()
    for a, b in zip((got[0], got[2], got[3]), (kept[0], kept[2], kept[3])):
        assert (bits(a) == bits(b)).all()


# ------------------------------------------------------------------------------------------------ 5. device cells
def test_adam_step_device_cells_three_launches(dev):
    """step_dev = {t - 1, ticket 0} and lr_dev in HBM; the host's step = 0 and lr = -1 are ignored, not refused.  Three launches
    without host-side arguments changing; lr_dev rewritten before the third takes effect."""
    lib = _lib.load()
    _, betas, eps, wd, t = R.HYPER_SETS[1]
    n = 4099
    lr32 = [np.float32(2e-3), np.float32(2e-3), np.float32(7e-4)]
    hyper = (float(lr32[0]), betas, eps, wd, t)
    p, g, m, v, plant = R.make_inputs(n, hyper, 90)
    slab = Slab(dev, n)
    slab.put(p, g, m, v)
    step_dev = torch.tensor([t - 1, 0], dtype=torch.int64, device=dev)
    lr_dev = torch.zeros(1, device=dev)
    for i in range(3):
        lr_dev.fill_(float(lr32[i]))
        h = (float(lr32[i]), betas, eps, wd, t + i)
        assert step(lib, slab, h, lr_dev=lr_dev, step_dev=step_dev, host_lr=-1.0, host_step=0) == 0
        got = slab.get()
        assert step_dev.tolist() == [t + i, 0]                      # published, the ticket re-armed
        check("device cells launch %d" % (i + 1), got, (p, g, m, v), h, plant if i == 0 else None)
        if i == 2:                                                  # ... and with the lr of the first two launches it would differ
            assert (bits(oracle(p, g, m, v, (float(lr32[0]),) + h[1:])[0]) != bits(got[0])).any()
        p, m, v = got[0], got[2], got[3]
        g = next_grad(g, p, hyper)
        slab.put(g=g)
    slab.guards_intact()


def test_adam_step_device_cells_through_8192_tickets(dev):
    """The aligned grid-stride size: 8 192 workgroups take a ticket, the last one publishes t and re-arms it."""
    lib = _lib.load()
    _, betas, eps, wd, t = R.HYPER_SETS[1]
    lr32 = np.float32(1.5e-3)
    hyper = (float(lr32), betas, eps, wd, t)
    n = N_VEC_STRIDE
    p, g, m, v, plant = R.make_inputs(n, hyper, 91)
    slab = Slab(dev, n)
    slab.put(p, g, m, v)
    step_dev = torch.tensor([t - 1, 0], dtype=torch.int64, device=dev)
    lr_dev = torch.full((1,), float(lr32), device=dev)
    assert step(lib, slab, hyper, lr_dev=lr_dev, step_dev=step_dev, host_lr=-1.0, host_step=0) == 0
    got = slab.get()
    assert step_dev.tolist() == [t, 0]
    slab.guards_intact()
    check("device cells, 8192 workgroups", got, (p, g, m, v), hyper, plant)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_adam_step_refusals_launch_nothing(dev):
    """Every case fails a host-side PN2_CHECK_ARG of pn2_adam_step before any launch; p, g, m, v and a step cell keep their bits."""
    lib = _lib.load()
    n = 64
    hyper = R.HYPER_SETS[1]
    p, g, m, v, _ = R.make_inputs(n, hyper, 95)
    slab = Slab(dev, n)
    slab.put(p, g, m, v)
    step_dev = torch.tensor([4, 0], dtype=torch.int64, device=dev)
    lr_dev = torch.full((1,), 1e-3, device=dev)
    st, nan = _lib.stream(), float("nan")
    ok = dict(n=n, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4, step=3, lr_dev=None, step_dev=None)

    def call(ptrs=slab.ptrs, **kw):
        a = dict(ok, **kw)
        return lib.pn2_adam_step(*ptrs, a["n"], a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step"], _lib.ptr(a["lr_dev"]),
                                 _lib.ptr(a["step_dev"]), 1, st)

    for i in range(4):                                              # a NULL pointer, one at a time
        assert call(ptrs=slab.ptrs[:i] + (None,) + slab.ptrs[i + 1:]) == EINVAL, i
    refused = [dict(n=0), dict(n=-5), dict(step=0), dict(step=-1), dict(b1=1.0), dict(b2=1.0), dict(b1=-0.1), dict(b2=-0.1),
               dict(eps=-1e-8), dict(wd=-1e-4), dict(lr=-1e-3), dict(lr=-1e-3, step_dev=step_dev),
               dict(lr=nan), dict(b1=nan), dict(b2=nan), dict(eps=nan), dict(wd=nan),
               dict(b1=nan, lr_dev=lr_dev, step_dev=step_dev), dict(eps=-1.0, lr_dev=lr_dev, step_dev=step_dev),
               dict(step=0, lr_dev=lr_dev)]
    for kw in refused:
        assert call(**kw) == EINVAL, kw
    got = slab.get()
    slab.guards_intact()
    for a, b, what in zip(got, (p, g, m, v), ("param", "grad", "exp_avg", "exp_avg_sq")):
        assert (bits(a) == bits(b)).all(), what                     # (zero_grad = 1 was asked for: the gradient was not cleared)
    assert step_dev.tolist() == [4, 0]
