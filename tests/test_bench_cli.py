"""bench.py's command line on a tiny workload: --steps sets the timed renders,
a plain run carries the headline fields and none of the --full legs, and
--dump-outputs writes the last timed step's accumulator, which equals the
oracle's render of that step's frames bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, STEPS, WARMUP = 64, 48, 2, 2, 1


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(oracle_scene, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--width", str(W), "--height", str(H), "--spp", str(SPP), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["steps"] == STEPS and j["warmup"] == WARMUP and j["full"] is False
    assert j["unit"] == "Mrays/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region (both are rounded to 3 decimals in the line)
    mrays = W * H * SPP / (j["ms_per_step"] * 1e-3) / 1e6
    assert abs(j["value"] - mrays) <= 2e-3 * mrays + 1e-3
    for k in ("roofline", "cpu_baseline", "parity", "gpu_vs_cpu", "kernel_ms_profile_pass"):
        assert j[k] is None, k
    assert sorted(os.listdir(out)) == ["accumulator.npy"]
    acc = np.load(out / "accumulator.npy")
    assert acc.dtype == np.float32 and acc.shape == (H, W, 4)
    first = (WARMUP + STEPS - 1) * SPP
    assert j["dumped_outputs"]["accumulator.npy"]["frames"] == [first, first + SPP]
    ref, _, _ = oracle_scene.render(W, H, SPP, first_frame=first)
    assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32))
