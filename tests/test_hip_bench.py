"""bench.py's plain run: the headline line alone, with the dumped outputs; everything else the benchmark measures comes with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a --full run adds to the line (bench.py docstring: "Extra objects on that line with --full")
FULL_ONLY = {"roofline", "fp16_mode", "w2_mode", "mixed_mode", "split_bf16_mode", "exact_fp32_mode", "parity_vs_fp32_reference",
             "eager_ms_per_step", "frozen_weights_ms_per_step", "frozen_weights_bit_identical", "sample_128_steps", "cpu_baseline",
             "train", "train_split_bf16", "configs", "upsample", "set_metrics"}


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_alone(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["metric"] == "denoiser_fwd_points_per_sec" and rec["unit"] == "points/s" and rec["higher_is_better"] is True
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["dtype"].startswith("f16/fp6/fp8")
    assert rec["value"] == pytest.approx(64 * 2048 / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert not FULL_ONLY & set(rec), sorted(FULL_ONLY & set(rec))
    den = np.load(tmp_path / "denoised.npy")
    assert den.shape == (64, 2048, 3) and np.isfinite(den).all()
