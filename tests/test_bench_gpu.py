"""GPU: a plain `bench.py` run is the headline only and times exactly --steps steps; --dump-outputs writes what the LAST timed
step returned -- its loss and log-probabilities from the same replay (the loss is the NLL of the dumped log-probabilities) --
and two runs with the same arguments write the same bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", "ssg",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_dumps_its_last_timed_step(dev, tmp_path):
    doc = _run(tmp_path / "a")
    assert doc["steps"] == 3 and doc["warmup"] == 2 and doc["ms_per_step"] > 0.0 and doc["value"] > 1e6
    assert doc["unit"] == "points/s" and doc["higher_is_better"] is True and doc["dtype"].startswith("f32")
    assert doc["roofline"] is None and doc["kernels"] is None and doc["cpu_baseline"] is None and "other_configs" not in doc

    from pointnet12_amd import synthetic as syn
    out = tmp_path / "a"
    assert sorted(os.listdir(out)) == ["log_probs.npy", "loss.npy"]
    lp, loss = np.load(out / "log_probs.npy"), np.load(out / "loss.npy")
    assert lp.dtype == np.float32 and lp.shape == (16, 4096, 13) and loss.shape == ()
    lp64 = lp.astype(np.float64).reshape(-1, 13)
    assert np.abs(np.exp(lp64).sum(1) - 1.0).max() <= 1e-4
    _, labels = syn.kitti_batch(0, 16, 4096)
    nll = -lp64[np.arange(lp64.shape[0]), labels.reshape(-1)].mean()
    assert abs(nll - float(loss)) <= 1e-5 * max(1.0, abs(nll))

    _run(tmp_path / "b")                                  # same arguments, same inputs: the same bits
    for f in ("log_probs.npy", "loss.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
