"""CPU: the generated gfx950 code of csrc/plane.hip uses no scratch (tools/check_isa.py, unchanged; hipcc cross-compiles without a
GPU): the scoring kernel's plane and count, the accumulate kernel's ten fp64 accumulators and the finish kernel's Jacobi sweeps on
scalars all stay in registers."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_plane_kernels_do_not_spill():
    assert os.path.exists(os.path.join(ROOT, "pointnet12_amd", "csrc", "plane.hip"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "plane.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
