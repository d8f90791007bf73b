"""bench.py --dump-outputs on the GPU: a plain run (no --full) of a small
ResNet-18 config writes what its last timed step returned, and writes the
same bits when run again; with --full the record also holds ps_parity."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(d, *more):
    return subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--model", "resnet18", "--batch", "16", "--image",
                           "64", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d), *more],
                          cwd=REPO, capture_output=True, text=True, timeout=300)


def test_bench_plain_run_dumps_last_step_outputs(gpu, tmp_path):
    d = tmp_path / "dump"
    p = _run(d)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["dtype"] == "bf16" and rec["higher_is_better"]
    assert abs(rec["value"] - 16 * 1e3 / rec["ms_per_step"]) <= 1e-2 * rec["value"]
    assert "ps_parity" not in rec  # only with --full
    assert rec["config"]["deterministic"] is True  # --deterministic auto: a dump run takes the reproducible kernels
    assert sorted(os.listdir(d)) == ["loss.npy", "out.npy"]
    out, loss = np.load(d / "out.npy"), np.load(d / "loss.npy")
    assert out.dtype == np.float32 and out.shape == (16, 1000) and np.isfinite(out).all() and out.std() > 0
    assert loss.dtype == np.float32 and abs(float(loss) - rec["config"]["final_loss"]) <= 1e-4
    d2 = tmp_path / "again"
    p = _run(d2, "--full")
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["ps_parity"]["ms_per_iter"] > 0 and "error" not in rec["ps_parity"]  # --full: the side benchmark ran
    assert np.array_equal(np.load(d2 / "out.npy"), out) and np.array_equal(np.load(d2 / "loss.npy"), loss)
