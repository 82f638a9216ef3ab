"""Inputs of the depth-visualisation tests and tests/golden/vis_reference.npz: what tests/helpers/vis_ref.py gives for them in float64.

    python tests/golden/make_vis_reference.py            # rewrites the fixture

The inputs are made here from seeds (the tests import this module for them); the fixture pins the float64 outputs so that a change of
the helper or of numpy shows up without a GPU (tests/test_vis_host.py) and the GPU tests compare against stored numbers.

range_case(shape): depths from random bit patterns (both signs, every byte of the sort key in use), +-inf, NaN and +-0 where the image
has room, about half of the pixels drawn from eight shared values so that long runs of equal depths exist; acc a multiple of 1 / 64
with zeros.  Every sum and both thresholds at ignore_frac 0.125 and 0.25 are then exact in float32 and float64.  For 15 pixels and
more the seed is advanced until a run of equal depths straddles the low and the high threshold at both fractions.
smooth_case(shape): depth uniform in (2, 6), acc fractional; the images the value / colour comparisons use, with bounds(shape).
mod_case(shape): depths whose -log(x + eps) stays 0.1 (k + u), u in [0.1, 0.9], away from the steps of the modular value at 0.1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "helpers"))
import vis_ref                       # noqa: E402

OUT = os.path.join(HERE, "vis_reference.npz")
SHAPES = [(1, 1), (3, 5), (37, 53), (130, 257)]
FRACS = [0.0, 0.125, 0.25]
STORED = SHAPES[:3]                       # full float64 planes; the largest case stores its ranges and colour indices only
F32 = np.float32


def name(shape):
    return f"{shape[0]}x{shape[1]}"


def _range_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    d = bits.view(F32).copy()
    bad = ~np.isfinite(d)
    d[bad] = F32(1.5) * (1 + np.arange(int(bad.sum()), dtype=F32))
    shared = d[rng.integers(0, n, 8)]
    pick = rng.uniform(size=n) < 0.5
    d[pick] = shared[rng.integers(0, 8, int(pick.sum()))]
    acc = (rng.integers(0, 65, n) / 64.0).astype(F32)
    acc[rng.uniform(size=n) < 0.1] = 0
    if n >= 15:
        special = rng.choice(n, 6, replace=False)
        d[special] = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, np.nan], F32)
    return d.reshape(shape), acc.reshape(shape)


def _straddles(d, acc, frac):
    """A run of equal depths holds a kept and a dropped pixel at the low end and at the high end."""
    flat, a = d.reshape(-1), np.where(np.isnan(d), 0, acc).reshape(-1).astype(np.float64)
    order = np.argsort(flat, kind="stable")
    ds, cum = flat[order], np.cumsum(a[order])
    keep = (cum >= cum[-1] * frac) & (cum <= cum[-1] * (1 - frac))
    k = np.flatnonzero(keep)
    if k.size == 0 or k[0] == 0 or k[-1] == flat.size - 1:
        return False
    return bool(ds[k[0] - 1] == ds[k[0]] and ds[k[-1] + 1] == ds[k[-1]] and a[order][k[0] - 1] != a[order][k[0]])


def range_case(shape):
    seed = 1000 * shape[0] + shape[1]
    if shape[0] * shape[1] < 15:
        return _range_inputs(shape, seed)
    for s in range(seed, seed + 500):
        d, acc = _range_inputs(shape, s)
        if all(_straddles(d, acc, f) for f in FRACS[1:]):
            return d, acc
    raise AssertionError(f"no seed gives straddling runs for {shape}")


def smooth_case(shape):
    rng = np.random.default_rng(7000 + 31 * shape[0] + shape[1])
    return rng.uniform(2, 6, shape).astype(F32), (rng.integers(0, 65, shape) / 64.0).astype(F32)


def bounds(shape):
    """near / far for the smooth case: automatic, except for one pixel alone (its own range is 2 eps wide: the value is all rounding)."""
    return dict(near=2.0, far=6.0) if shape == (1, 1) else {}


def mod_case(shape):
    rng = np.random.default_rng(9000 + 31 * shape[0] + shape[1])
    k, u = rng.integers(-17, -7, shape), rng.uniform(0.1, 0.9, shape)
    return (np.exp(-0.1 * (k + u)) - vis_ref.EPS).astype(F32), (rng.integers(0, 65, shape) / 64.0).astype(F32)


def outputs(shape):
    """name -> float64 array, for one shape."""
    out = {}
    d, acc = range_case(shape)
    for f in FRACS:
        out[f"range_{f}"] = np.array(vis_ref.auto_range(d, acc, f), np.float64)
    d, acc = smooth_case(shape)
    dep = vis_ref.visualize_depth(d, acc, **bounds(shape))
    out["index"] = dep["index"].astype(np.uint8)
    if shape in STORED:
        out["value"], out["depth"] = dep["value"], dep["rgb"]
        out["depth_mod"] = vis_ref.visualize_depth(d, acc, modulus=0.1)["rgb"]
        out["depth_normals"], out["normals"], s = vis_ref.visualize_normals(d, acc)
        out["scaling"] = np.float64(s)
        md, macc = mod_case(shape)
        out["mod_value"] = vis_ref.visualize_depth(md, macc, modulus=0.1)["value"]
    return out


def build():
    return {f"{name(s)}/{k}": v for s in SHAPES for k, v in outputs(s).items()}


if __name__ == "__main__":
    np.savez_compressed(OUT, **build())
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    for s in SHAPES:
        d, acc = smooth_case(s)
        i32 = vis_ref.visualize_depth(d, acc, dtype=F32, **bounds(s))["index"]
        i64 = vis_ref.visualize_depth(d, acc, **bounds(s))["index"]
        print(f"{name(s)}: turbo index float32 vs float64 differs on {int((i32 != i64).sum())} of {i64.size} pixels")
