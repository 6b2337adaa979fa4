"""CPU: the Chamfer drop-in contract (pointnet12_amd/chamfer.py against the reference's model/chamfer.py, recorded in
tests/golden/g15_chamfer.npz by tools/make_golden_chamfer.py).  The fp64 restatement (tests/chamfer_ref.py) is held against every
recorded case -- that is what ties the yardstick of tests/test_chamfer_gpu.py to the reference -- and the checks that need no
device are exercised: the public names, the reference's asserts and IndexError, CPU tensors, the ABI 14 entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import chamfer_ref as C

from pointnet12_amd import _lib


def cases():
    g = golden("g15_chamfer.npz")
    return g, [str(c) for c in g["cases"]]


def test_public_names():
    from pointnet12_amd import chamfer as M
    for name in ("chamfer_batch", "chamfer_non_batch", "num", "nearest_neighbor", "chamfer_symmetric"):
        assert callable(getattr(M, name)), name
    x = torch.arange(6.0).reshape(2, 3).requires_grad_(True)
    assert isinstance(M.num(x), np.ndarray) and M.num(x).tolist() == [[0, 1, 2], [3, 4, 5]]


def test_checks_come_before_any_launch():
    from pointnet12_amd import chamfer as M
    z = torch.zeros
    with pytest.raises(AssertionError):
        M.chamfer_batch(z(2, 4, 3), z(3, 4, 3))              # B differs
    with pytest.raises(AssertionError):
        M.chamfer_batch(z(2, 4, 3), z(2, 4, 2))              # D differs
    with pytest.raises(AssertionError):
        M.chamfer_non_batch(z(2, 4, 3), z(2, 4, 3))          # B != 1
    with pytest.raises(AssertionError):
        M.chamfer_non_batch(z(1, 4, 3), z(1, 4, 4))
    with pytest.raises(IndexError):
        M.chamfer_batch(z(2, 4, 3), z(2, 0, 3))              # the reference's min() over an empty dimension
    for fn in (M.chamfer_batch, M.chamfer_symmetric, M.nearest_neighbor):
        with pytest.raises(_lib.Pn2Error):
            fn(z(2, 4, 3), z(2, 5, 3))                       # CPU tensors: this package has no CPU path
    with pytest.raises(_lib.Pn2Error):
        M.chamfer_non_batch(z(1, 4, 3), z(1, 5, 3))


def test_restatement_against_the_reference():
    g, names = cases()
    assert {"main", "rand3", "d2", "d4", "d6", "d9", "subset", "tie3", "nonbatch"} <= set(names)
    assert "%.4f" % float(g["main/value"]) == "11.6073"                    # the number the reference's own __main__ prints
    for c in names:
        p1, p2 = torch.from_numpy(g[c + "/p1"]), torch.from_numpy(g[c + "/p2"])
        assert p1.dtype == torch.float32 and p2.dtype == torch.float32
        gr, B = float(g[c + "/g"]), p1.shape[0]
        assert gr != 1.0
        if str(g[c + "/fn"]) == "chamfer_non_batch":
            assert B == 1
        ref_idx = torch.from_numpy(g[c + "/argmin"].astype(np.int64))
        d64, i64 = C.nearest(p1, p2)
        assert bool((i64 == ref_idx).all()), c
        # the REFERENCE's numbers are held to the very bounds the HIP results have to meet against this restatement
        fig = C.check_against(p1, p2, gr, None, ref_idx, torch.from_numpy(g[c + "/value"]), torch.from_numpy(g[c + "/dp1"]),
                              torch.from_numpy(g[c + "/dp2"]), exact_idx=ref_idx, what=c)
        print(c, fig)
        if c + "/gap" in g:
            assert float(g[c + "/gap"]) >= 1e-5 and abs(C.nearest_gap(p1, p2) - float(g[c + "/gap"])) <= 1e-12


def test_fixture_pins_zero_rows_and_ties():
    g, _ = cases()
    d64, i64 = C.nearest(torch.from_numpy(g["subset/p1"]), torch.from_numpy(g["subset/p2"]))
    zero = d64 == 0
    assert int(zero.sum()) >= 100 and bool((torch.from_numpy(g["subset/dp1"])[zero] == 0).all())      # torch.norm's backward at 0
    p2 = g["subset/p2"]
    twins = sum(len(p2[b]) - len(np.unique(p2[b], axis=0)) for b in range(p2.shape[0]))
    assert twins > 0                                                                                 # exact ties at distance 0
    assert g["tie3/argmin"].tolist() == [[1, 1, 4, 4]]                                               # lowest index, not first seen
    assert np.array_equal(g["tie3/dp2"][0, 2:4], np.zeros((2, 3), np.float32)) and np.abs(g["tie3/dp2"][0, 1]).max() > 0
    assert np.array_equal(g["tie3/dp2"][0, 5], np.zeros(3, np.float32))


def test_abi_14_entry_points():
    text = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+15\b", text) and _lib.ABI_VERSION == 15
    for name in ("pn2_chamfer_nn", "pn2_chamfer_nn_workspace_bytes", "pn2_chamfer_bwd"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, text), name
    lib = _lib.load()
    assert lib.pn2_version() == 15
    # argument checks and the workspace query are host code: no GPU needed
    assert lib.pn2_chamfer_nn(None, None, 1, 1, 1, 3, None, None, None, None, None) == -1
    assert lib.pn2_chamfer_bwd(None, None, None, None, None, 1, 1, 1, 3, None, None, None) == -1
    one = ctypes.c_void_p(256)                                # a non-NULL placeholder: refused shapes launch nothing
    assert lib.pn2_chamfer_nn(one, one, 1, 8, 8, 17, one, one, None, one, None) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_chamfer_bwd(one, one, one, one, one, 1, 8, 8, 17, one, one, None) == _lib.PN2_EUNSUPPORTED
    assert lib.pn2_chamfer_nn(one, one, 1, 8, 0, 3, one, one, None, one, None) == -1
    for shape in ((16, 4096, 4096, 3), (1, 2048, 2048, 3), (1, 1, 1, 1), (8, 65536, 65536, 3), (1, 65536, 8192, 16)):
        nbytes = lib.pn2_chamfer_nn_workspace_bytes(*shape)
        B, N, M, D = shape
        assert 0 < nbytes < 4 * B * N * M or N * M < 4096, shape      # never anything of size N x M
        assert nbytes <= 64 << 20, (shape, nbytes)
    assert lib.pn2_chamfer_nn_workspace_bytes(1, 8, 8, 17) == 0
    # the workspace query takes no stream: the call-profile proxy must hand it out unwrapped
    with _lib.call_profile():
        assert _lib._lib.pn2_chamfer_nn_workspace_bytes(1, 2048, 2048, 3) == lib.pn2_chamfer_nn_workspace_bytes(1, 2048, 2048, 3)
