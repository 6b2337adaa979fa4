"""CPU: the generated gfx950 code of csrc/feature_match.hip and csrc/corr_ransac.hip uses no scratch (tools/check_isa.py, unchanged;
hipcc cross-compiles without a GPU): pn2_feature_nn2 keeps a query row of 36 or 64 floats and its two slots in registers,
pn2_corr_ransac twelve doubles per hypothesis, pn2_corr_refit seventeen accumulators and the 4 x 4 Jacobi solve (csrc/sym_eig4.h:
every index a compile-time constant)."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
@pytest.mark.parametrize("name", ["feature_match.hip", "corr_ransac.hip"])
def test_matching_kernels_do_not_spill(name):
    assert os.path.exists(os.path.join(ROOT, "pointnet12_amd", "csrc", name))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", name], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
