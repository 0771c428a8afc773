"""bench.py without --full: the headline line and --dump-outputs, nothing measured after the timed steps (the roofline
leg, the per-kernel breakdown, the extras and the CPU baseline belong to --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_only(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["unit"] == "crops/s" and line["higher_is_better"] is True and line["steps"] == 3
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 32e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    assert line["dtype"].startswith("bf16x6") and line["config"]["per_gpu_batch"] == 32
    assert line["full"] is False
    for block in ("roofline", "kernel_breakdown", "extras", "cpu_baseline"):
        assert line[block] is None, block
    kp = np.load(tmp_path / "keypoints.npy")
    assert kp.shape == (32, 11, 3) and kp.dtype == np.float32 and np.isfinite(kp).all()
