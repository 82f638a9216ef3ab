"""bench.py's --dump-outputs writer and its options, on the CPU side: float32 (float64 kept) .npy files, the 64 MB bound, and a sample of the
same rows in every run when an output is larger than its share (the GPU side: tests/test_gpu_bench_outputs.py)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_writes_float_arrays_by_name(tmp_path):
    arrays = {"params": torch.arange(1000, dtype=torch.float32), "stats_loss": torch.tensor(0.25), "stats_psnr": np.float64(6.0),
              "count": torch.arange(4, dtype=torch.int32), "rgb": torch.rand(16, 3, dtype=torch.float64)}
    bench.dump_outputs(arrays, str(tmp_path / "out"))
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == set(arrays)
    assert got["params"].dtype == np.float32 and np.array_equal(got["params"], np.arange(1000, dtype=np.float32))
    assert got["count"].dtype == np.float32 and got["stats_loss"].dtype == np.float32 and float(got["stats_loss"].reshape(-1)[0]) == 0.25
    assert got["rgb"].dtype == np.float64 and np.array_equal(got["rgb"], arrays["rgb"].numpy())


def test_dump_stays_below_64_mb_with_the_same_rows_every_run(tmp_path):
    g = torch.Generator().manual_seed(3)
    arrays = {"small": torch.ones(10), "wide": torch.rand(6_000_000, 4, generator=g), "flat": torch.rand(9_000_000, generator=g)}
    for d in ("a", "b"):
        bench.dump_outputs(arrays, str(tmp_path / d))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000, total
    wide = np.load(tmp_path / "a" / "wide.npy")
    assert wide.shape[1] == 4 and 0 < wide.shape[0] < 6_000_000
    assert np.isin(wide[:, 0], arrays["wide"].numpy()[:, 0]).all()           # whole rows of the output, not a resampling
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), np.ones(10, np.float32))
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_bench_has_the_full_and_dump_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
