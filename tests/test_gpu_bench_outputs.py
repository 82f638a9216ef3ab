"""A plain `bench.py` run (no --full) end to end: the headline fields only, exactly --steps timed steps, and --dump-outputs writing what the
last timed step computed — the training state and the step's statistics, or every level of the render pass — from the same inputs in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(extra, dump):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "example", "--rays", "256",
           "--dump-outputs", str(dump)] + extra
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "rays/s" and d["higher_is_better"] is True and d["n_gpus"] == 1
    assert abs(d["value"] - 256 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "roofline_march", "sustained_mfma", "stability", "frame", "cpu_baseline", "parity", "variants", "precision_legs"):
        assert k not in d, k                                  # measured behind --full only
    return d, {f[:-4]: np.load(os.path.join(dump, f)) for f in sorted(os.listdir(dump))}


@pytest.mark.timeout(1200)
def test_plain_train_run_dumps_the_training_state(tmp_path):
    d, a = _bench([], tmp_path / "a")
    assert d["metric"] == "rays/sec (train step)" and d["dtype"] == "f16x3/fp32-acc"
    assert {"params", "adam_mu", "adam_nu", "grads", "stats_loss", "stats_psnr"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) < 64_000_000
    assert a["params"].ndim == 1 and a["grads"].size > a["params"].size and np.isfinite(a["params"]).all() and float(a["stats_loss"].reshape(-1)[0]) > 0
    _, b = _bench([], tmp_path / "b")
    assert set(a) == set(b)
    for k in a:                                               # same arguments, same inputs: the same step to fp32 rounding
        np.testing.assert_allclose(a[k], b[k], rtol=1e-4, atol=1e-6, err_msg=k)


@pytest.mark.timeout(600)
def test_plain_forward_run_dumps_every_level(tmp_path):
    d, a = _bench(["--mode", "forward"], tmp_path / "f")
    assert d["metric"] == "rays/sec (forward render pass)"
    assert a["coarse_comp_rgb"].shape == (256, 3) and a["coarse_distance"].shape == (256,) and a["coarse_trans_rgb_bkgd"].shape == (256, 3)
    assert all(np.isfinite(v).all() for v in a.values())
