"""bench.py command line: the result line and --dump-outputs."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def test_bench_options_listed():
    proc = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--help"],
        capture_output=True, text=True, timeout=60,
    )
    assert proc.returncode == 0, proc.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full",
                "--seed"):
        assert opt in proc.stdout


@pytest.mark.gpu
def test_bench_dump_outputs_gpu(tmp_path):
    """One short plain run: the result line carries ms_per_step for the
    requested number of steps, and the dumped array is what the last
    step's requests returned (one (8, 1000) float32 block per slot;
    every slot is fed the same input, so every block must agree)."""
    from client_amd.ops import gpu_available

    if not gpu_available():
        pytest.skip("no HIP device")
    proc = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--concurrency", "4", "--reqs-per-step", "8",
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=300, cwd=tmp_path,
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    assert result["steps"] == 2
    assert result["ms_per_step"] > 0
    assert result["unit"] == "inferences/sec"
    # value and ms_per_step describe the same timed window
    per_step = 8 * 8  # reqs_per_step * batch
    assert result["value"] == pytest.approx(
        per_step / (result["ms_per_step"] / 1e3), rel=1e-3)

    assert [p.name for p in tmp_path.glob("*.npy")] == ["output0.npy"]
    out = np.load(tmp_path / "output0.npy")
    assert out.dtype == np.float32
    assert out.shape == (4, 8, 1000)
    assert np.all(np.isfinite(out))
    assert out.std() > 0
    # same input in every slot; the dynamic batcher may run a request at
    # a different batch size, which can pick another conv kernel, so
    # blocks agree to bf16 rounding through the network, not bitwise
    scale = np.abs(out).max()
    assert np.abs(out - out[0]).max() <= 0.05 * scale
