"""CPU: the generated gfx950 code of csrc/normals.hip uses no scratch (tools/check_isa.py, unchanged; hipcc cross-compiles without a
GPU): one row per lane with nine fp64 accumulators, the 3 x 3 Jacobi solve on scalars, and the unrolled slot groups all stay in
registers.  The packed-fp32 check of tests/test_isa_cpu.py disassembles the whole built library, this file's kernels included."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_normals_kernels_do_not_spill():
    assert os.path.exists(os.path.join(ROOT, "pointnet12_amd", "csrc", "normals.hip"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "scratch", "normals.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
