"""CPU: the generated gfx950 code of csrc/fpfh.hip uses no scratch (tools/check_isa.py, unchanged; hipcc cross-compiles without a
GPU): pn2_spfh keeps its 33 run-time indexed counters in LDS and the rotating slot loads in registers, pn2_fpfh its 33 fp64
accumulators and two packed neighbour rows in registers with every index a compile-time constant."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_fpfh_kernels_do_not_spill():
    assert os.path.exists(os.path.join(ROOT, "pointnet12_amd", "csrc", "fpfh.hip"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "fpfh.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
