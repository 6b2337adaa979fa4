"""CPU: the arithmetic pn2_sgd_step must have (tests/sgd_ref.py) IS torch.optim.SGD's, bit for bit; the header, the ctypes table
and the built library carry the entry point; optim.SGD's constructor refuses what torch's refuses and has no CPU fallback."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sgd_ref as R
from conftest import ROOT
from pointnet12_amd import _lib, optim


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", [1, 7, 1027, 100003])
@pytest.mark.parametrize("opts", R.OPTION_SETS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "plain")
def test_restatement_is_torch_sgd_bit_for_bit(opts, n):
    """12 steps, lr changed in the loop (param_group['lr'] as pcdseg.py:159-163 rewrites it), gradients over five decades."""
    gen = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=gen)
    tp = torch.nn.Parameter(p0.clone())
    ref = torch.optim.SGD([tp], lr=0.01, **opts)
    p, buf = p0.numpy().copy(), None
    p64, buf64 = p.astype(np.float64), None
    for t in range(1, 13):
        lr = 0.01 * 0.7 ** (t // 3) * (1.0 + 0.1 * (t % 2))
        ref.param_groups[0]["lr"] = lr
        grad = torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=gen))
        tp.grad = grad.clone()
        ref.step()
        buf = R.sgd_step(p, grad.numpy(), buf, t, lr, **opts)
        buf64 = R.sgd_step64(p64, grad.numpy(), buf64, t, lr, **opts)
        assert (bits(p) == bits(tp.detach().numpy())).all(), t
        if opts.get("momentum", 0) != 0:
            assert (bits(buf) == bits(ref.state[tp]["momentum_buffer"].numpy())).all(), t
        else:
            assert buf is None and "momentum_buffer" not in ref.state[tp]
    # a check that sgd_step64 states the same rule, not an error bound: 12 steps of fp32 rounding (2^-24 ~ 6e-8 each, the
    # momentum sum amplifying a buffer's by at most 1/(1 - 0.9)) stay well below 1e-5 of the parameters' scale
    assert np.abs(p - p64).max() <= 1e-5 * max(np.abs(p64).max(), 1.0)


def test_header_and_binding_table_declare_sgd_step():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+15\b", text) and _lib.ABI_VERSION == 15
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+pn2_sgd_step\s*\(", text, flags=re.S)
    assert m and "pn2_sgd_step (added within ABI 15: purely additive, no version change)" in " ".join(m.group(1).split())
    res, args = _lib.SIGNATURES["pn2_sgd_step"]
    assert res is ctypes.c_int and len(args) == 15
    assert args[3] is ctypes.c_int64 and args[4:8] == [ctypes.c_double] * 4 and args[8:10] == [ctypes.c_int] * 2
    lib = _lib.load()
    assert hasattr(lib, "pn2_sgd_step") and lib.pn2_version() == 15


def test_argument_checks_need_no_gpu():
    """Refused before anything touches the device: no pointers, n = 0 (the GPU test repeats these with real buffers)."""
    lib = _lib.load()
    assert lib.pn2_sgd_step(None, None, None, 4, 0.01, 0.0, 0.0, 0.0, 0, 0, 1, None, None, 0, None) == -1
    assert lib.pn2_sgd_step(16, 16, None, 0, 0.01, 0.0, 0.0, 0.0, 0, 0, 1, None, None, 0, None) == -1
    assert lib.pn2_sgd_step(16, 16, None, 4, 0.01, 0.9, 0.0, 0.0, 0, 0, 1, None, None, 0, None) == -1      # momentum, no buffer
    assert lib.pn2_sgd_step(16, 16, 16, 4, 0.01, 0.9, 0.1, 0.0, 1, 0, 1, None, None, 0, None) == -1        # nesterov + dampening
    assert lib.pn2_sgd_step(16, 16, 16, 4, 0.01, 0.0, 0.0, 0.0, 1, 0, 1, None, None, 0, None) == -1        # nesterov, no momentum
    assert lib.pn2_sgd_step(16, 16, 16, 4, -0.01, 0.9, 0.0, 0.0, 0, 0, 1, None, None, 0, None) == -1
    assert lib.pn2_sgd_step(16, 16, 16, 4, 0.01, -0.9, 0.0, 0.0, 0, 0, 1, None, None, 0, None) == -1
    assert lib.pn2_sgd_step(16, 16, 16, 4, 0.01, 0.9, 0.0, -1e-4, 0, 0, 1, None, None, 0, None) == -1
    assert lib.pn2_sgd_step(16, 16, 16, 4, 0.01, 0.9, 0.0, 0.0, 0, 0, 0, None, None, 0, None) == -1        # step 0, no device cell


def test_constructor_refuses_what_torch_refuses():
    one = lambda: [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-0.1), dict(momentum=-0.5), dict(weight_decay=-1e-4), dict(nesterov=True),
               dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError) as theirs:
            torch.optim.SGD(one(), **kw)
        with pytest.raises(ValueError) as ours:
            optim.SGD(one(), **kw)
        assert str(ours.value) == str(theirs.value), kw
    with pytest.raises(NotImplementedError):
        optim.SGD(one(), differentiable=True)
    with pytest.raises(_lib.Pn2Error):
        optim.SGD(one(), lr=0.01, momentum=0.9)                   # CPU parameters: no fallback
    with pytest.raises(_lib.Pn2Error):
        optim.SGD(one(), foreach=True, fused=False)               # accepted and ignored: still refused for the device alone
