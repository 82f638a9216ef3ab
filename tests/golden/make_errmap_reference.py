"""Golden vectors computed BY THE REFERENCE's own text for metric/summary.py's error maps: tests/golden/errmap_reference.npz.

    python tests/golden/make_errmap_reference.py [out.npz]      # needs the reference, CPU torch and scipy; commits only recorded data

Nothing is imported from the reference and nothing of it is copied into this repository.  Per image pair the script runs
  * metric/ssim/ssim.py as it stands (pure torch), compiled from its text, through SSIM(data_range=1.0) as summary.py:115 builds it;
  * compute_psnr, compute_ssim and save_err of metric/summary.py:43-61, read out of the source with `ast` (summary.py imports cv2,
    lpips and imageio at the top, so it cannot be imported), with `flip` bound to CHWtoHWC, index2color and get_magma_map read out of
    metric/flip/data.py the same way (data.py imports OpenEXR) and `imageio.imsave` bound to a function that keeps the array;
  * compute_ldrflip through tests/golden/make_flip_reference.py (its float64 and float32 accumulations),
on float32 inputs made here from seeds, and records the inputs, the float32 maps and values, the coloured bytes of each map and the
256 x 3 colour bytes (save_err on a map whose value at i is (i + 0.5) / 255).

Two measured kinds of number go with them, and the tolerances of tests/test_gpu_errmap.py rest on them:
  e_ref_<map>_<case>: the largest |reference float32 map - float64 map| on that input (float64: tests/helpers/errmap_ref.py for the
      squared error and SSIM; the float64 accumulation of make_flip_reference for FLIP);
  share_<map>_<case>: the share of pixels whose colour index differs between the reference's float32 map and that float64 map.
The script refuses inputs on which that share exceeds 1 % or an index differs by more than 1 (the end-to-end condition of the tests),
and a blurred pair whose SSIM map does not span most of its range.

Pairs: 11 x 11 (one window), 29 x 33 (69 flat output columns: the channel triple at flat columns 63-65 straddles the 64-column tile;
19 output rows, more than a row tile; the test image is a blurred copy of the reference), 45 x 70 (values outside [0, 1])."""
import ast
import hashlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "helpers"))
import errmap_ref                    # noqa: E402
import make_flip_reference as MF     # noqa: E402

REF = MF.REF                                              # RNERF_REFERENCE_ROOT
SRC_SSIM = os.path.join(REF, "metric", "ssim", "ssim.py")
SRC_SUMMARY = os.path.join(REF, "metric", "summary.py")
SRC_DATA = os.path.join(REF, "metric", "flip", "data.py")
OUT = os.path.join(HERE, "errmap_reference.npz")
CASES = ("11x11", "29x33", "45x70")
MAPS = ("psnr", "ssim", "flip")
PPD = 0.3 * (400 / 0.5) * np.pi / 180                      # metric/summary.py:72-75
F32 = np.float32


def inputs():
    """case -> (reference, test), float32 [H, W, 3]."""
    rng = np.random.default_rng(20261019)

    def smooth(h, w, phase):
        y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        return np.stack([0.5 + 0.3 * np.sin(5 * x + c + phase) * np.cos(4 * y - c) for c in range(3)], -1)

    out = {}
    a = 0.6 * smooth(11, 11, 0.3) + 0.4 * rng.uniform(0, 1, (11, 11, 3))
    out["11x11"] = (a, np.clip(a + 0.08 * rng.standard_normal(a.shape), 0, 1))
    # a textured image and its blur, sharp on the left and more and more blurred to the right: SSIM from near 1 downwards
    a = np.clip(0.5 * smooth(29, 33, 1.0) + 0.5 * rng.uniform(0, 1, (29, 33, 3)), 0, 1)
    pad = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
    blur = sum(pad[i:i + 29, j:j + 33] for i in range(3) for j in range(3)) / 9.0
    t = np.linspace(0, 1, 33)[None, :, None]
    out["29x33"] = (a, (1 - t) * a + t * blur + 0.002)
    a = 1.5 * smooth(45, 70, 2.0) - 0.2 + 0.1 * rng.standard_normal((45, 70, 3))
    out["45x70"] = (a, a + 0.15 * rng.standard_normal(a.shape))
    return {k: (np.ascontiguousarray(r, F32), np.ascontiguousarray(t, F32)) for k, (r, t) in out.items()}


def _functions(path, names):
    raw = open(path, "rb").read()
    tree = ast.parse(raw.decode(), path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    if sorted(f.name for f in fns) != sorted(names) or any(f.decorator_list for f in fns):
        raise RuntimeError(f"{path}: expected exactly one undecorated definition of each of {names}")
    return ast.Module(body=fns, type_ignores=[]), hashlib.sha256(raw).hexdigest()


def reference_functions():
    """-> (namespace with ssim_model, compute_psnr, compute_ssim, save_err and `saved`, {file: sha256}); (None, None) without the reference."""
    if not all(os.path.exists(p) for p in (SRC_SSIM, SRC_SUMMARY, SRC_DATA)):
        return None, None
    import torch
    sha = {}
    raw = open(SRC_SSIM, "rb").read()
    sha["ssim"] = hashlib.sha256(raw).hexdigest()
    ssim_ns = {"__name__": "reference_ssim"}
    exec(compile(raw.decode(), SRC_SSIM, "exec"), ssim_ns)
    mod, sha["data"] = _functions(SRC_DATA, ("CHWtoHWC", "index2color", "get_magma_map"))
    data_ns = {"np": np}
    exec(compile(mod, SRC_DATA, "exec"), data_ns)
    saved = []
    mod, sha["summary"] = _functions(SRC_SUMMARY, ("compute_psnr", "compute_ssim", "save_err"))
    ns = {"np": np, "torch": torch, "flip": types.SimpleNamespace(**{k: data_ns[k] for k in ("CHWtoHWC", "index2color", "get_magma_map")}),
          "imageio": types.SimpleNamespace(imsave=lambda fpath, img: saved.append(np.array(img)))}
    exec(compile(mod, SRC_SUMMARY, "exec"), ns)
    ns["ssim_model"] = ssim_ns["SSIM"](data_range=1.0)                              # summary.py:115, on the CPU
    ns["saved"] = saved
    return ns, sha


def compute(ns):
    """name -> array, everything the fixture holds but the hashes."""
    import torch
    flip_fns, _ = MF.reference_compute_ldrflip()

    def save_err(m):
        ns["save_err"]("unused.png", m)
        return ns["saved"].pop()

    arrays = {}
    lut_in = ((np.arange(256, dtype=np.float64) + 0.5) / 255.0).astype(F32).reshape(16, 16)
    arrays["lut"] = save_err(lut_in).reshape(256, 3)
    assert arrays["lut"].dtype == np.uint8
    for case, (ref, test) in inputs().items():
        rb, tb = (torch.FloatTensor(x).permute(2, 0, 1)[None] for x in (ref, test))        # summary.py:207-208
        with torch.no_grad():
            psnr_val, psnr_map = ns["compute_psnr"](rb, tb)
            ssim_raw_val, ssim_raw = ns["ssim_model"](rb, tb)
            ssim_val, ssim_map = ns["compute_ssim"](ns["ssim_model"], rb, tb)
        ssim_raw = ssim_raw.squeeze().cpu().numpy().reshape(ref.shape[0] - 10, ref.shape[1] - 10)
        ssim_map = ssim_map.reshape(ssim_raw.shape)
        chw = lambda x: np.ascontiguousarray(x.transpose(2, 0, 1))
        with np.errstate(invalid="ignore"):
            flip32, flip64 = (np.asarray(flip_fns[acc](chw(ref), chw(test), PPD))[0] for acc in (np.float32, np.float64))
        flip_map = flip64.astype(F32)                                                     # as tests/golden/flip_reference.npz stores it
        mse64, mse = errmap_ref.mse_map(ref, test)
        ssim64, ssim64_val = errmap_ref.ssim_summary(ref, test)
        assert np.array_equal(np.clip(ssim_raw, 0, 1), ssim_map) and float(ssim_raw_val) == ssim_val
        assert ssim_raw.min() < 0.5 and ssim_raw.max() > 0.9 or case != "29x33", (case, ssim_raw.min(), ssim_raw.max())
        arrays[f"in_{case}_ref"], arrays[f"in_{case}_test"] = ref, test
        arrays[f"map_psnr_{case}"], arrays[f"map_ssim_{case}"], arrays[f"map_flip_{case}"] = psnr_map.astype(F32), ssim_raw.astype(F32), flip_map
        arrays[f"value_psnr_{case}"], arrays[f"value_ssim_{case}"] = np.float64(psnr_val), np.float64(ssim_val)
        arrays[f"value_flip_{case}"] = np.float64(np.mean(flip_map))                      # summary.py:78
        arrays[f"value64_psnr_{case}"], arrays[f"value64_ssim_{case}"] = np.float64(errmap_ref.psnr_value(mse)), np.float64(ssim64_val)
        pairs = {"psnr": (psnr_map, mse64), "ssim": (ssim_raw, ssim64), "flip": (flip32, flip64)}
        for name, colour_in in (("psnr", psnr_map), ("ssim", ssim_map), ("flip", flip_map)):
            arrays[f"bytes_{name}_{case}"] = save_err(colour_in)
            m32, m64 = pairs[name]
            arrays[f"e_ref_{name}_{case}"] = np.float64(np.max(np.abs(m32.astype(np.float64) - m64)))
            i32, i64 = errmap_ref.map_index(m32.astype(F32)), errmap_ref.map_index(m64.astype(F32))
            share = float(np.mean(i32 != i64))
            assert np.max(np.abs(i32 - i64)) <= 1 and share <= 0.01, f"{case} {name}: pick other inputs (share {share})"
            arrays[f"share_{name}_{case}"] = np.float64(share)
    return arrays


def main(path=OUT):
    ns, sha = reference_functions()
    if ns is None:
        print(f"SKIPPED: {REF}/metric is not on this machine")
        return None
    arrays = compute(ns)
    for k, v in sha.items():
        arrays[f"source_sha256_{k}"] = np.array(v)
    np.savez_compressed(path, **arrays)
    for case in CASES:
        print(case, {n: (float(arrays[f"e_ref_{n}_{case}"]), float(arrays[f"share_{n}_{case}"])) for n in MAPS},
              "ssim range", float(arrays[f"map_ssim_{case}"].min()), float(arrays[f"map_ssim_{case}"].max()))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    return path


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
