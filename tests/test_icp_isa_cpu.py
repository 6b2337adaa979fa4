"""CPU: the generated gfx950 code of csrc/icp.hip uses no scratch (tools/check_isa.py, unchanged; hipcc cross-compiles without a
GPU): the accumulate kernel's 28 fp64 accumulators beside the walk's state, and the finish kernel's 6 x 6 Cholesky solve and
rotation update on scalars all stay in registers."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_icp_kernels_do_not_spill():
    assert os.path.exists(os.path.join(ROOT, "pointnet12_amd", "csrc", "icp.hip"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "icp.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
