"""CPU: pn2_cross_entropy_* (pcdseg.py:178-179) are declared, bound and exported, refuse bad arguments before anything touches
the device, and loss.cross_entropy refuses what it cannot run; there is no CPU fallback."""
import ctypes

import pytest
import torch

from pointnet12_amd import _lib
from pointnet12_amd.loss import CrossEntropyLoss, cross_entropy

EINVAL = -1
NAMES = ("pn2_cross_entropy_workspace_bytes", "pn2_cross_entropy_fwd", "pn2_cross_entropy_bwd")


def test_binding_table_and_library_carry_the_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    res, args = _lib.SIGNATURES["pn2_cross_entropy_fwd"]
    assert res is ctypes.c_int and len(args) == 15 and args[8] is ctypes.c_double
    res, args = _lib.SIGNATURES["pn2_cross_entropy_bwd"]
    assert res is ctypes.c_int and len(args) == 15 and args[9] is ctypes.c_double
    assert lib.pn2_version() == _lib.ABI_VERSION                  # added within the current ABI: no version change


def _fwd(lib, x=16, ld=8, inner=0, target=16, R=4, C=5, eps=0.0, reduction=1, ws=16, lse=16, loss=16, denom=16):
    return lib.pn2_cross_entropy_fwd(x, ld, inner, target, None, R, C, -100, eps, reduction, ws, lse, loss, denom, None)


def _bwd(lib, x=16, ld=8, inner=0, target=16, lse=16, R=4, C=5, eps=0.0, reduction=1, grad=16, denom=16, dx=16):
    return lib.pn2_cross_entropy_bwd(x, ld, inner, target, None, lse, R, C, -100, eps, reduction, grad, denom, dx, None)


def test_argument_checks_need_no_gpu():
    """Every call below is refused before a launch (the non-null pointers are never dereferenced)."""
    lib = _lib.load()
    assert lib.pn2_cross_entropy_workspace_bytes(0) == EINVAL and lib.pn2_cross_entropy_workspace_bytes(-3) == EINVAL
    assert lib.pn2_cross_entropy_workspace_bytes(1) == lib.pn2_cross_entropy_workspace_bytes(10 ** 7) > 0
    for call in (_fwd, _bwd):
        for null in ("x", "target", "lse"):
            assert call(lib, **{null: None}) == EINVAL, (call.__name__, null)
        assert call(lib, C=0) == EINVAL
        assert call(lib, C=65, ld=68) == EINVAL
        assert call(lib, C=5, ld=4) == EINVAL                      # ld < C
        assert call(lib, R=0) == EINVAL
        assert call(lib, reduction=3) == EINVAL and call(lib, reduction=-1) == EINVAL
        assert call(lib, eps=-0.1) == EINVAL and call(lib, eps=1.5) == EINVAL and call(lib, eps=float("nan")) == EINVAL
        assert call(lib, inner=-1) == EINVAL
        assert call(lib, R=10, inner=4) == EINVAL                  # [B, C, inner]: R must be B * inner
    assert _fwd(lib, loss=None) == EINVAL
    assert _fwd(lib, reduction=1, ws=None) == EINVAL and _fwd(lib, reduction=2, denom=None) == EINVAL
    assert _bwd(lib, grad=None) == EINVAL and _bwd(lib, dx=None) == EINVAL
    assert _bwd(lib, reduction=1, denom=None) == EINVAL


def test_cross_entropy_refuses_what_it_cannot_run():
    x, t = torch.randn(6, 5), torch.randint(0, 5, (6,))
    with pytest.raises(_lib.Pn2Error, match="must be a GPU tensor"):
        cross_entropy(x, t)                                        # CPU tensors: no fallback
    with pytest.raises(_lib.Pn2Error, match="must be a GPU tensor"):
        CrossEntropyLoss()(torch.randn(2, 7, 5).transpose(2, 1), torch.randint(0, 5, (2, 7)))
    with pytest.raises(_lib.Pn2Error, match="65 classes"):
        cross_entropy(torch.randn(6, 65), t)
    for bad in (torch.randn(6, 10)[:, ::2],                        # classes two floats apart
                torch.randn(6, 1).expand(6, 5),                    # stride 0
                torch.randn(7, 2, 5).permute(1, 2, 0),             # [B, C, N] with n the slowest
                torch.randn(2, 5, 14)[:, :, ::2]):                 # class-strided, n two floats apart
        with pytest.raises(_lib.Pn2Error, match="neither row-major"):
            cross_entropy(bad, torch.zeros(bad.shape[:1] + bad.shape[2:], dtype=torch.int64))
    with pytest.raises(TypeError):
        cross_entropy(x.double(), t)
    for eps in (-0.01, 1.01):
        with pytest.raises(ValueError):
            cross_entropy(x, t, label_smoothing=eps)
    with pytest.raises(ValueError):
        cross_entropy(x, t, reduction="average")
    for n in (4, 6):
        with pytest.raises(ValueError):
            cross_entropy(x, t, weight=torch.ones(n))
    with pytest.raises(ValueError):
        cross_entropy(x, t[:5])                                    # 6 rows, 5 targets
    with pytest.raises(ValueError):
        cross_entropy(torch.randn(2, 5, 7), torch.randint(0, 5, (2, 5)))
    with pytest.raises(NotImplementedError):
        cross_entropy(x, torch.softmax(x, -1))                     # class-probability targets: out of scope


def test_layouts_read_in_place():
    """(rows, pitch, inner) as the wrapper hands them to the kernels, from strides alone."""
    from pointnet12_amd.loss import _ce_layout as L
    assert L(torch.empty(6, 5)) == (6, 5, 0)
    assert L(torch.empty(6, 8)[:, :5]) == (6, 8, 0)                            # a column slice of a padded buffer
    assert L(torch.empty(6, 8)[:, 1:6]) == (6, 8, 0)
    assert L(torch.empty(2, 7, 19).transpose(2, 1)) == (14, 19, 0)             # pcdseg.py:178
    assert L(torch.empty(2, 7, 20)[:, :, :19].transpose(2, 1)) == (14, 20, 0)
    assert L(torch.empty(1, 7, 19).transpose(2, 1)) == (7, 19, 0) and L(torch.empty(2, 1, 19).transpose(2, 1)) == (2, 19, 0)
    assert L(torch.empty(2, 3, 4, 5).permute(0, 3, 1, 2)) == (24, 5, 0)
    assert L(torch.empty(2, 19, 7)) == (14, 0, 7) and L(torch.empty(2, 5, 3, 4)) == (24, 0, 12)
    assert L(torch.empty(5, 6).t()) == (6, 0, 6)                               # [R, C] whose transpose is contiguous: B = 1
    assert L(torch.empty(1, 5)) == (1, 5, 0) and L(torch.empty(3, 1)) == (3, 1, 0)
    assert L(torch.empty(2, 7, 19)[::2].transpose(2, 1)) == (7, 19, 0)
    assert L(torch.empty(4, 7, 19)[::2].transpose(2, 1)) is None               # the clouds do not collapse into one run of rows


def test_module_takes_torchs_constructor_arguments():
    w = torch.rand(5)
    m = CrossEntropyLoss(weight=w, size_average=None, ignore_index=3, reduce=None, reduction="sum", label_smoothing=0.1)
    ref = torch.nn.CrossEntropyLoss(weight=w, ignore_index=3, reduction="sum", label_smoothing=0.1)
    assert (m.ignore_index, m.reduction, m.label_smoothing) == (ref.ignore_index, ref.reduction, ref.label_smoothing)
    assert torch.equal(m.weight, ref.weight) and "weight" in dict(m.named_buffers())
    assert CrossEntropyLoss().weight is None and CrossEntropyLoss().reduction == "mean"
