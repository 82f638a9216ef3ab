"""Golden vectors computed BY THE REFERENCE's own SSIM text: utils.compute_ssim (rnerf/utils.py:404-471).

rnerf/utils.py cannot be imported here (it imports jax), but compute_ssim only needs a few array functions.  This script reads the
compute_ssim FunctionDef out of the reference's source with `ast` (nothing is imported from the reference, nothing of it is copied into
this repository), compiles it as it stands, and calls it with a whitelist of builtins and three stand-ins:
  jnp                      numpy, with `mean` taking a list of axes as jnp.mean does
  jsp.signal.convolve2d    scipy.signal.convolve2d
  jax.vmap(f, in_axes, out_axes)   a loop over the mapped axis (np.take), stacked and moved to out_axes
The arithmetic is float64 on float32-representable inputs: the yardstick the device kernel is held to.  Inputs, outputs and the source's
sha256 go to tests/golden/ssim_reference.npz — data, not source.  tests/test_ssim_host.py checks the float64 restatement
(tests/helpers/ssim_ref.py) against the file and re-runs this script wherever the reference is present; tests/test_gpu_ssim.py holds
rnerf_ssim to it.

usage: python tests/golden/make_ssim_reference.py [out.npz] | --check"""
import ast
import hashlib
import os
import sys
import types

import numpy as np

REF = os.environ.get("RNERF_REFERENCE_ROOT", "/root/reference")
SRC = os.path.join(REF, "rnerf", "utils.py")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ssim_reference.npz")

_b = __builtins__ if isinstance(__builtins__, dict) else vars(__builtins__)
SAFE_BUILTINS = {k: _b[k] for k in ("range", "len", "int", "float", "list", "tuple", "min", "max", "abs")}


def _numpy_only_import(name, *args, **kwargs):
    """numpy / scipy import their own submodules lazily through the calling frame's builtins: allow exactly that."""
    if name.split(".")[0] not in ("numpy", "scipy"):
        raise ImportError(f"compute_ssim may import numpy / scipy only, not {name!r}")
    import builtins
    return builtins.__import__(name, *args, **kwargs)


SAFE_BUILTINS["__import__"] = _numpy_only_import


def source_sha256():
    return hashlib.sha256(open(SRC, "rb").read()).hexdigest() if os.path.exists(SRC) else None


def _stand_ins():
    import scipy.signal

    def mean(a, axis=None):
        return np.mean(a, axis=tuple(axis) if isinstance(axis, list) else axis)

    jnp = types.SimpleNamespace(arange=np.arange, exp=np.exp, sum=np.sum, maximum=np.maximum, minimum=np.minimum, sign=np.sign,
                                sqrt=np.sqrt, abs=np.abs, mean=mean)
    jsp = types.SimpleNamespace(signal=types.SimpleNamespace(convolve2d=scipy.signal.convolve2d))

    def vmap(f, in_axes=0, out_axes=0):
        def g(z):
            return np.moveaxis(np.stack([f(np.take(z, i, axis=in_axes)) for i in range(z.shape[in_axes])], 0), 0, out_axes)
        return g

    return {"jnp": jnp, "jsp": jsp, "jax": types.SimpleNamespace(vmap=vmap)}


def reference_compute_ssim(expect_sha256=None):
    """compute_ssim compiled from the reference's text; None when the reference is not on this machine.  The file's hash is taken BEFORE
    anything of it is compiled; with `expect_sha256` a file that is not the one the fixture was made from is refused unexecuted."""
    if not os.path.exists(SRC):
        return None, None
    raw = open(SRC, "rb").read()
    sha = hashlib.sha256(raw).hexdigest()
    if expect_sha256 is not None and sha != expect_sha256:
        raise RuntimeError(f"{SRC}: sha256 {sha[:16]} is not the source the committed vectors were made from ({expect_sha256[:16]}): "
                           "nothing of it was executed; re-run tests/golden/make_ssim_reference.py after reading the diff")
    tree = ast.parse(raw.decode(), SRC)
    for fn in (n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_ssim"):
        if fn.decorator_list:
            raise RuntimeError(f"{SRC}: compute_ssim carries a decorator: refusing to execute it")
        ns = {"__builtins__": dict(SAFE_BUILTINS), **_stand_ins()}
        exec(compile(ast.Module(body=[fn], type_ignores=[]), SRC, "exec"), ns)
        return ns["compute_ssim"], sha
    raise RuntimeError(f"{SRC}: compute_ssim not found")


def _f32(a):
    return np.asarray(a, np.float32)


def inputs():
    """input set -> (img0, img1), float32 (what the device kernel reads)."""
    rng = np.random.default_rng(20261016)
    base0, base1 = _f32(rng.uniform(0, 1, (2, 24, 31, 3))), _f32(rng.uniform(0, 1, (2, 24, 31, 3)))
    sm0 = _f32(rng.uniform(0, 1, (13, 17, 2)))
    sm1 = _f32(0.6 * sm0 + 0.4 * rng.uniform(0, 1, (13, 17, 2)))
    mono0, mono1 = _f32(rng.uniform(0, 1, (17, 23, 1))), _f32(rng.uniform(0, 1, (17, 23, 1)))
    nan0, nan1 = _f32(rng.uniform(0, 1, (15, 16, 3))), _f32(rng.uniform(0, 1, (15, 16, 3)))
    nan0[7, 9, 1] = np.nan
    return {"base": (base0, base1), "small": (sm0, sm1), "small255": (_f32(np.round(sm0 * 255)), _f32(np.round(sm1 * 255))),
            "affine_negative": (sm0, _f32(-0.7 * sm0.astype(np.float64) + 0.9)), "mono_odd": (mono0, mono1), "nan": (nan0, nan1)}


# case -> (input set, keyword arguments of compute_ssim)
CASES = {
    "default": ("base", {"max_val": 1.0}),
    "default_map": ("base", {"max_val": 1.0, "return_map": True}),
    "fs1": ("small", {"max_val": 1.0, "filter_size": 1, "return_map": True}),
    "fs4": ("small", {"max_val": 1.0, "filter_size": 4, "return_map": True}),
    "fs7_sigma0p8": ("small", {"max_val": 1.0, "filter_size": 7, "filter_sigma": 0.8, "return_map": True}),
    "maxval255": ("small255", {"max_val": 255.0, "filter_size": 5, "k1": 0.02, "k2": 0.05, "return_map": True}),
    "affine_negative": ("affine_negative", {"max_val": 1.0, "filter_size": 5, "return_map": True}),
    "mono_odd": ("mono_odd", {"max_val": 1.0, "return_map": True}),
    "nan": ("nan", {"max_val": 1.0, "filter_size": 5, "return_map": True}),
}


def compute(fn):
    x = inputs()
    out = {}
    for name, (src, kw) in CASES.items():
        a, b = x[src]
        out[name] = np.asarray(fn(a.astype(np.float64), b.astype(np.float64), **kw), np.float64)
    return out


def main(path=OUT):
    fn, sha = reference_compute_ssim()
    if fn is None:
        print(f"SKIPPED: {SRC} is not on this machine")
        return None
    arrays = {"source_sha256": np.array(sha)}
    for src, (a, b) in inputs().items():
        arrays[f"in_{src}_0"], arrays[f"in_{src}_1"] = a, b
    for name, y in compute(fn).items():
        arrays[f"out_{name}"] = y
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(CASES)} cases computed by {SRC} (sha256 {sha[:16]})")
    return path


def check(path=OUT):
    """`--check`: the committed vectors are what the reference computes today — same source hash, same bits."""
    if source_sha256() is None:
        raise SystemExit(f"{SRC} is not on this machine: nothing to check against")
    d = np.load(path)
    fn, _ = reference_compute_ssim(expect_sha256=str(d["source_sha256"]))
    again = compute(fn)
    bad = [k for k, y in again.items() if not np.array_equal(y, d[f"out_{k}"], equal_nan=True)]
    bad += [k for k, (a, b) in inputs().items() if not (np.array_equal(a, d[f"in_{k}_0"], equal_nan=True)
                                                        and np.array_equal(b, d[f"in_{k}_1"], equal_nan=True))]
    print(f"{path}: " + ("equals what the reference computes, bit for bit" if not bad else "DIFFERS in " + ", ".join(bad)))
    return not bad


if __name__ == "__main__":
    if sys.argv[1:] == ["--check"]:
        raise SystemExit(0 if check() else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
