"""CPU: a process that loads libpn2_hip.so BEFORE it imports torch itself (``python __graft_entry__.py smoke`` does, through
``build()``) still ends up with ONE HIP runtime.  torch's ROCm wheel carries its own libamdhip64.so under a file name that is not
the SONAME the library asks for, so the dynamic loader maps a second runtime when the library comes first, and launches on
torch's streams then fail with PN2_ELAUNCH; ``_lib.load()`` therefore imports torch before it opens the library.  The order is the
whole point, hence the fresh interpreter."""
import subprocess
import sys

from conftest import ROOT

SCRIPT = """
import sys
sys.path.insert(0, %r)
from pointnet12_amd import _lib
assert "torch" not in sys.modules
_lib.load()
import torch
print(len({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l}))
"""


def test_library_first_maps_one_hip_runtime():
    r = subprocess.run([sys.executable, "-c", SCRIPT % ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.strip().splitlines()[-1]) == 1, r.stdout
