"""What tests/test_flip_host.py and tests/test_gpu_flip.py share: loading a vector of tests/golden/flip_reference.npz and holding a FLIP
map to it.  The rules and where their numbers come from are stated in tests/test_flip_host.py's docstring."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_flip_reference as M      # noqa: E402
import flip_ref                      # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "flip_reference.npz")


def load_case(key):
    """-> reference, test, ppd, expected map (float64), floor, floor_mean."""
    d = np.load(FIXTURE)
    case, p = key.rsplit("_", 1)
    a, b = M.case_inputs(M.load_base(d))[case]
    return a, b, M.PPD[p], d[f"out_{key}"].astype(np.float64), float(d[f"floor_{key}"]), float(d[f"floor_mean_{key}"])


def identical_footprint(a, b, radius):
    """[..., H, W] bool: every pixel within `radius` (border replicated) is bit-identical in a and b.  NaN differs from everything."""
    diff = np.any(a.view(np.uint32) != b.view(np.uint32), axis=-1) | np.any(np.isnan(a) | np.isnan(b), axis=-1)
    H, W = diff.shape[-2:]
    pad = np.pad(diff, [(0, 0)] * (diff.ndim - 2) + [(radius, radius)] * 2, mode="edge")
    hit = np.zeros_like(diff)
    for i in range(2 * radius + 1):
        for j in range(2 * radius + 1):
            hit |= pad[..., i:i + H, j:j + W]
    return ~hit


def check_against_fixture(key, got_map, got_mean=None):
    """The rules of this file's docstring for one fixture vector; returns (max error / floor, mean error) for the record."""
    a, b, ppd, want, floor, floor_mean = load_case(key)
    got_map = np.asarray(got_map, np.float64)
    assert got_map.shape == want.shape
    assert np.array_equal(np.isnan(got_map), np.isnan(want)), f"{key}: NaN mask"
    ok = ~np.isnan(want)
    e_max = float(np.max(np.abs(got_map - want)[ok]))
    img_axes = (-2, -1)
    e_mean = float(np.max(np.abs(np.mean(np.where(ok, got_map, 0), img_axes) - np.mean(np.where(ok, want, 0), img_axes))))
    print(f"{key}: max error {e_max:.3g} (floor {floor:.3g}, ratio {e_max / floor:.3g}); mean error {e_mean:.3g} "
          f"(bound {2 * floor_mean + 1e-6:.3g})")
    if key.rsplit("_", 1)[0] in M.CLASS_A:
        assert e_max <= 4 * floor + 1e-6, f"{key}: map error {e_max:.3g} vs floor {floor:.3g}"
    else:
        zero = identical_footprint(a, b, max(flip_ref.radii(ppd)))
        assert zero.any() or key.startswith("nan")
        assert np.all(got_map[zero] == 0.0), f"{key}: {int(np.sum(got_map[zero] != 0))} non-zero values where the footprints are identical"
    assert e_mean <= 2 * floor_mean + 1e-6, f"{key}: mean error {e_mean:.3g}"
    if got_mean is not None:
        got_mean = np.asarray(got_mean, np.float64)
        assert got_mean.shape == want.shape[:-2]
        full = np.mean(want, img_axes)
        assert np.array_equal(np.isnan(got_mean), np.isnan(full))
        fin = ~np.isnan(full)
        assert np.all(np.abs(got_mean - full)[fin] <= 2 * floor_mean + 1e-6), f"{key}: returned mean {got_mean} vs {full}"
    return e_max / floor, e_mean
