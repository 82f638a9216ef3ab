"""Golden vectors computed BY THE REFERENCE's own LDR-FLIP text: compute_ldrflip (metric/flip/flip_api.py:134-495).

metric/flip/flip_api.py cannot be imported here (it imports cv2, and through data.py OpenEXR and Imath), but compute_ldrflip only needs
numpy and one cv2 call.  This script reads the FunctionDefs compute_ldrflip needs out of the reference's source with `ast` (nothing is
imported from the reference, nothing of it is copied into this repository), compiles them as they stand, and runs them with numpy as
`np`, the `sys` module, a whitelist of builtins, and ONE stand-in that is ours, not the reference's:
  cv.filter2D(img, ddepth=-1, kernel=k, borderType=cv.BORDER_REPLICATE)
      scipy.ndimage.correlate(img, k, mode="nearest"), accumulating in float64, cast back to img's dtype.
The images go in as float32 [3, H, W], as metric/summary.py:49-78 passes them, so every other step is the reference's float32 arithmetic.

For every case the text is run a second time with the stand-in accumulating in float32 (tap by tap, weights rounded to float32):
  floor_<case>      = max  |out_f32acc - out|
  floor_mean_<case> = mean |out_f32acc - out|
are the float32 noise of the reference's own pipeline on that input, and every tolerance of tests/test_flip_host.py and
tests/test_gpu_flip.py is built from them.

Inputs are 8-bit images (stored as uint8, value / 255 in float32), so the file stays small; outputs are stored as float32.  Class A cases
differ everywhere; class B cases are identical on part of the image, where the metric's last step deltaE_c ^ (1 - deltaE_f) is
ill-conditioned (a tiny non-zero colour difference), so only their mean, their exact zeros and their NaN mask are held to the file.
Inputs, outputs, floors and the source's sha256 go to tests/golden/flip_reference.npz — data, not source.

usage: python tests/golden/make_flip_reference.py [out.npz] | --check"""
import ast
import hashlib
import os
import sys
import types

import numpy as np

REF = os.environ.get("RNERF_REFERENCE_ROOT", "/root/reference")
SRC = os.path.join(REF, "metric", "flip", "flip_api.py")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flip_reference.npz")

PPD = {"lo": 0.3 * (400 / 0.5) * np.pi / 180,            # metric/summary.py:72-75: 4.189, radii 1 and 1
       "hi": (0.7 * 3840 / 0.7) * np.pi / 180}           # compute_ldrflip's default: 67.02, radii 10 and 9
NEEDED = ("color_space_transform", "generate_spatial_filter", "spatial_filter", "hunt_adjustment", "hyab", "redistribute_errors",
          "feature_detection", "compute_ldrflip")
CLASS_A = ("noise", "smooth_noised", "batch")
CLASS_B = ("half_identical", "nan")
NAN_AT = (20, 37, 1)                                      # (row, column, channel) of the reference image's one NaN

_b = __builtins__ if isinstance(__builtins__, dict) else vars(__builtins__)
SAFE_BUILTINS = {k: _b[k] for k in ("range", "len", "int", "float", "list", "tuple", "min", "max", "abs")}


def _numpy_only_import(name, *args, **kwargs):
    """numpy / scipy import their own submodules lazily through the calling frame's builtins: allow exactly that."""
    if name.split(".")[0] not in ("numpy", "scipy"):
        raise ImportError(f"compute_ldrflip may import numpy / scipy only, not {name!r}")
    import builtins
    return builtins.__import__(name, *args, **kwargs)


SAFE_BUILTINS["__import__"] = _numpy_only_import


def source_sha256():
    return hashlib.sha256(open(SRC, "rb").read()).hexdigest() if os.path.exists(SRC) else None


def filter2d_stand_in(acc_dtype):
    """OUR stand-in for cv2.filter2D with BORDER_REPLICATE (correlation, anchor at the kernel's centre).  float64: scipy.ndimage.correlate
    on the image as float64.  float32: the same sum tap by tap in float32, weights rounded to float32 (scipy always accumulates in
    double).  Either way the result is cast back to the image's dtype."""
    import scipy.ndimage

    def filter2D(img, ddepth=-1, kernel=None, borderType=None):
        assert ddepth == -1 and borderType == "replicate" and img.ndim == 2
        if acc_dtype == np.float64:
            return scipy.ndimage.correlate(img.astype(np.float64), np.asarray(kernel, np.float64), mode="nearest").astype(img.dtype)
        r = kernel.shape[0] // 2
        H, W = img.shape
        pad = np.pad(img.astype(np.float32), r, mode="edge")
        k = np.asarray(kernel, np.float32)
        acc = np.zeros((H, W), np.float32)
        for i in range(kernel.shape[0]):
            for j in range(kernel.shape[1]):
                acc += k[i, j] * pad[i:i + H, j:j + W]
        return acc.astype(img.dtype)

    return types.SimpleNamespace(filter2D=filter2D, BORDER_REPLICATE="replicate")


def reference_compute_ldrflip(expect_sha256=None):
    """{acc dtype: compute_ldrflip} compiled from the reference's text, and the file's sha256; (None, None) when the reference is not on
    this machine.  The hash is taken BEFORE anything of the file is compiled; with `expect_sha256` a file that is not the one the fixture
    was made from is refused unexecuted."""
    if not os.path.exists(SRC):
        return None, None
    raw = open(SRC, "rb").read()
    sha = hashlib.sha256(raw).hexdigest()
    if expect_sha256 is not None and sha != expect_sha256:
        raise RuntimeError(f"{SRC}: sha256 {sha[:16]} is not the source the committed vectors were made from ({expect_sha256[:16]}): "
                           "nothing of it was executed; re-run tests/golden/make_flip_reference.py after reading the diff")
    tree = ast.parse(raw.decode(), SRC)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NEEDED]
    if sorted(f.name for f in fns) != sorted(NEEDED):
        raise RuntimeError(f"{SRC}: expected exactly one definition of each of {NEEDED}")
    if any(f.decorator_list for f in fns):
        raise RuntimeError(f"{SRC}: a function compute_ldrflip needs carries a decorator: refusing to execute it")
    out = {}
    for acc in (np.float64, np.float32):
        ns = {"__builtins__": dict(SAFE_BUILTINS), "np": np, "sys": sys, "cv": filter2d_stand_in(acc)}
        exec(compile(ast.Module(body=fns, type_ignores=[]), SRC, "exec"), ns)
        out[acc] = ns["compute_ldrflip"]
    return out, sha


def _u8(a):
    return np.clip(np.round(np.asarray(a) * 255), 0, 255).astype(np.uint8)


def base_images():
    """The stored images, uint8 [H, W, 3] (or [2, H, W, 3] for the batch)."""
    rng = np.random.default_rng(20261017)
    H, W = 48, 64

    def smooth(h, w, phase):
        y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        return np.stack([0.5 + 0.35 * np.sin(3 * x + c + phase) * np.cos(2 * y - c) for c in range(3)], -1)

    sm = smooth(H, W, 0.0)
    small = smooth(24, 32, 1.0)
    return {"noise_0": _u8(rng.uniform(0, 1, (H, W, 3))), "noise_1": _u8(rng.uniform(0, 1, (H, W, 3))),
            "smooth": _u8(sm), "smooth_noised": _u8(sm + 0.05 * rng.standard_normal((H, W, 3))),
            "batch_0": np.stack([_u8(rng.uniform(0, 1, (24, 32, 3))), _u8(small)]),
            "batch_1": np.stack([_u8(rng.uniform(0, 1, (24, 32, 3))), _u8(small + 0.05 * rng.standard_normal((24, 32, 3)))])}


def case_inputs(base):
    """case -> (reference, test), float32 [..., H, W, 3], from the stored images (a mapping with base_images()' keys) by indexing alone."""
    def f32(u):
        return np.asarray(u, np.uint8).astype(np.float32) / np.float32(255)
    sm, smn = f32(base["smooth"]), f32(base["smooth_noised"])
    half = smn.copy()
    half[:, :half.shape[1] // 2] = sm[:, :half.shape[1] // 2]
    nan_ref = sm.copy()
    nan_ref[NAN_AT] = np.nan
    return {"noise": (f32(base["noise_0"]), f32(base["noise_1"])), "smooth_noised": (sm, smn),
            "batch": (f32(base["batch_0"]), f32(base["batch_1"])), "half_identical": (sm, half), "nan": (nan_ref, smn)}


def keys():
    return [f"{case}_{p}" for case in CLASS_A + CLASS_B for p in PPD]


def compute(fns):
    """key -> (out float32, floor, floor_mean)."""
    x = case_inputs(base_images())
    res = {}
    for case, (a, b) in x.items():
        for p, ppd in PPD.items():
            pairs = [(a, b)] if a.ndim == 3 else list(zip(a, b))
            o = {}
            with np.errstate(invalid="ignore"):
                for acc, fn in fns.items():
                    o[acc] = np.stack([np.asarray(fn(np.ascontiguousarray(r.transpose(2, 0, 1)), np.ascontiguousarray(t.transpose(2, 0, 1)),
                                                     ppd), np.float64)[0] for r, t in pairs])
            out = o[np.float64] if a.ndim == 4 else o[np.float64][0]
            d = np.abs((o[np.float32] if a.ndim == 4 else o[np.float32][0]) - out)
            ok = ~np.isnan(out)
            assert np.array_equal(np.isnan(d), ~ok)
            res[f"{case}_{p}"] = (out.astype(np.float32), float(np.max(d[ok])), float(np.mean(d[ok])))
    return res


def main(path=OUT):
    fns, sha = reference_compute_ldrflip()
    if fns is None:
        print(f"SKIPPED: {SRC} is not on this machine")
        return None
    arrays = {"source_sha256": np.array(sha)}
    for k, v in base_images().items():
        arrays[f"in_{k}"] = v
    for k, (out, floor, floor_mean) in compute(fns).items():
        arrays[f"out_{k}"], arrays[f"floor_{k}"], arrays[f"floor_mean_{k}"] = out, np.float64(floor), np.float64(floor_mean)
        print(f"{k}: mean {np.nanmean(out):.6f}, floor {floor:.3g}, floor_mean {floor_mean:.3g}")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(keys())} vectors computed by {SRC} (sha256 {sha[:16]}), {os.path.getsize(path)} bytes")
    return path


def load_base(d):
    return {k[3:]: d[k] for k in d.files if k.startswith("in_")}


def check(path=OUT):
    """`--check`: the committed vectors are what the reference computes today — same source hash, same bits."""
    if source_sha256() is None:
        raise SystemExit(f"{SRC} is not on this machine: nothing to check against")
    d = np.load(path)
    fns, _ = reference_compute_ldrflip(expect_sha256=str(d["source_sha256"]))
    bad = [k for k, (out, floor, floor_mean) in compute(fns).items()
           if not (np.array_equal(out, d[f"out_{k}"], equal_nan=True) and floor == float(d[f"floor_{k}"])
                   and floor_mean == float(d[f"floor_mean_{k}"]))]
    bad += [k for k, v in base_images().items() if not np.array_equal(v, d[f"in_{k}"])]
    print(f"{path}: " + ("equals what the reference computes, bit for bit" if not bad else "DIFFERS in " + ", ".join(bad)))
    return not bad


if __name__ == "__main__":
    if sys.argv[1:] == ["--check"]:
        raise SystemExit(0 if check() else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
