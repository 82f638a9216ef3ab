"""Golden vectors computed BY THE REFERENCE: its scene loaders on the tiny scenes of tests/helpers/scene_fixture.py.

rnerf/datasets.py cannot be imported here (module-level `import jax` and `import cv2`), but at `factor: 0` these methods touch neither:
  Blender._load_renderings (:334-370)    NSVF._load_renderings (:376-423)    OpenCV._load_renderings (:429-464)
  OpenCV._next_test (:466-484), on the rays of OpenCV._generate_rays (:486-518)
As tests/golden/make_from_reference_numpy.py does, this script takes the hash of the reference's files first, reads those FunctionDefs out
of its source with `ast`, compiles each as it stands with a whitelist of builtins, and calls it with a plain attribute holder as `self`;
`utils.open_file` is the builtin `open`, and `json`, `os`, `path`, `glob`, PIL's `Image` and `np` are handed in.  Nothing is imported from
the reference and none of its text is copied: inputs (the scenes, written fresh from their seeds) and outputs go to
tests/golden/scene_loader_reference.npz — data.  Cases: white_bkgd on / off, skip_frames 1 / 2, eval_train, an RGB OpenCV scene, and the
test crop with and without precrop_iters.  `factor: 2` needs cv2 and is not run: its expected values come from the definition
(include/rnerf.h, scene_fixture.prepare_reference).

usage: python tests/golden/make_scene_loader_reference.py [out.npz] | --check"""
import ast
import glob as glob_module
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_from_reference_numpy as base      # noqa: E402
import scene_fixture                          # noqa: E402

OUT = os.path.join(HERE, "scene_loader_reference.npz")
WANTED = {("Blender", "_load_renderings"), ("NSVF", "_load_renderings"), ("OpenCV", "_load_renderings"), ("OpenCV", "_next_test"),
          ("OpenCV", "_generate_rays")}
PRECROP_FRAC = 0.5


def _numpy_pil_import(name, *args, **kwargs):
    if name.split(".")[0] not in ("numpy", "PIL"):
        raise ImportError(f"the reference's loaders may import numpy and PIL only, not {name!r}")
    import builtins
    return builtins.__import__(name, *args, **kwargs)


def reference_methods(expect_sha256=None):
    """{(class, method): function} compiled from the reference's text, and the hash of its files; ({}, None) without the reference.  The hash
    is taken — and with expect_sha256 compared — before anything is compiled."""
    sha = base.source_sha256()
    if sha is None:
        return {}, None
    if expect_sha256 is not None and sha != expect_sha256:
        raise RuntimeError(f"{base.SRC}: sha256 {sha[:16]} is not the source the committed vectors were made from ({expect_sha256[:16]}): "
                           "nothing of it was executed")
    tree = ast.parse(open(base.SRC, "rb").read().decode(), base.SRC)
    builtins_ = dict(base.SAFE_BUILTINS)
    builtins_.update(open=open, map=map, sorted=sorted, ValueError=ValueError, NotImplementedError=NotImplementedError,
                     __import__=_numpy_pil_import)
    utils = types.SimpleNamespace(open_file=open, Rays=base.Rays, namedtuple_map=base._reference_namedtuple_map())
    out = {}
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef)):
        for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
            if (cls.name, fn.name) in WANTED:
                if fn.decorator_list:
                    raise RuntimeError(f"{base.SRC}: {cls.name}.{fn.name} carries a decorator: refusing to execute it")
                ns = {"__builtins__": dict(builtins_), "np": np, "utils": utils, "json": json, "os": os, "path": os.path,
                      "glob": glob_module.glob, "Image": Image}
                exec(compile(ast.Module(body=[fn], type_ignores=[]), base.SRC, "exec"), ns)
                out[(cls.name, fn.name)] = ns[fn.name]
    missing = WANTED - set(out)
    if missing:
        raise RuntimeError(f"{base.SRC}: methods not found: {sorted(missing)}")
    return out, sha


# name -> (scene, class, split, flags)
CASES = {
    "blender_test": ("blender", "Blender", "test", {}),
    "blender_test_white": ("blender", "Blender", "test", dict(white_bkgd=True)),
    "blender_train_skip2": ("blender", "Blender", "train", dict(skip_frames=2)),
    "blender_test_eval_train": ("blender", "Blender", "test", dict(eval_train=True)),
    "opencv_test": ("opencv", "OpenCV", "test", {}),
    "opencv_test_white": ("opencv", "OpenCV", "test", dict(white_bkgd=True)),
    "opencv_train_skip2": ("opencv", "OpenCV", "train", dict(skip_frames=2)),
    "opencv_test_eval_train": ("opencv", "OpenCV", "test", dict(eval_train=True)),
    "opencv_rgb_test": ("opencv_rgb", "OpenCV", "test", {}),
    "nsvf_test": ("nsvf", "NSVF", "test", {}),
    "nsvf_test_white": ("nsvf", "NSVF", "test", dict(white_bkgd=True)),
    "nsvf_train": ("nsvf", "NSVF", "train", {}),
}
CROPS = {"opencv_crop_off": 0, "opencv_crop_on": 2}      # name -> precrop_iters, on the scene and flags of "opencv_test"


def write_scenes(root):
    """The scenes every case reads, under `root` -> {scene: directory}."""
    dirs = {k: os.path.join(root, k) for k in ("blender", "opencv", "opencv_rgb", "nsvf")}
    scene_fixture.write_blender(dirs["blender"])
    scene_fixture.write_opencv(dirs["opencv"])
    scene_fixture.write_opencv(dirs["opencv_rgb"], channels=3)
    scene_fixture.write_nsvf(dirs["nsvf"])
    return dirs


def flags_of(data_dir, **over):
    f = dict(data_dir=data_dir, render_path=False, eval_train=False, skip_frames=1, factor=0, white_bkgd=False)
    f.update(over)
    return types.SimpleNamespace(**f)


def compute(meth):
    out = {}
    with tempfile.TemporaryDirectory() as root:
        dirs = write_scenes(root)
        loaded = {}
        for name, (scene, cls, split, over) in CASES.items():
            me = types.SimpleNamespace(split=split)
            meth[(cls, "_load_renderings")](me, flags_of(dirs[scene], **over))
            loaded[name] = me
            out[f"{name}_images"] = np.asarray(me.images)
            out[f"{name}_camtoworlds"] = np.asarray(me.camtoworlds)
            out[f"{name}_h"], out[f"{name}_w"], out[f"{name}_n_examples"] = np.array(me.h), np.array(me.w), np.array(me.n_examples)
            if cls == "OpenCV":
                out[f"{name}_cam_mat"] = np.array(me.cam_mat, np.float64)
            else:
                out[f"{name}_focal"] = np.array(me.focal, np.float64)
        for name, precrop_iters in CROPS.items():
            me = loaded["opencv_test"]
            me.use_pixel_centers = False
            meth[("OpenCV", "_generate_rays")](me)
            me.test_it, me.precrop_iters, me.precrop_frac, me.render_path = 0, precrop_iters, PRECROP_FRAC, False
            for call in range(me.n_examples + 1):                    # one more than there are views: the wrap-around
                b = meth[("OpenCV", "_next_test")](me)
                out[f"{name}_{call}_pixels"] = np.ascontiguousarray(b["pixels"])
                out[f"{name}_{call}_origins"] = np.ascontiguousarray(b["rays"].origins)
                out[f"{name}_{call}_viewdirs"] = np.ascontiguousarray(b["rays"].viewdirs)
    return out


def main(path=OUT):
    meth, sha = reference_methods()
    if not meth:
        print(f"SKIPPED: {base.SRC} is not on this machine")
        return None
    y = compute(meth)
    np.savez_compressed(path, source_sha256=np.array(sha), **y)
    print(f"wrote {path}: {len(y)} arrays computed by {base.SRC} (sha256 {sha[:16]}), {os.path.getsize(path)} bytes")
    return path


def check(path=OUT):
    """The committed vectors are what the reference computes today on freshly written scenes: same source hash, same bits."""
    if base.source_sha256() is None:
        raise SystemExit(f"{base.SRC} is not on this machine: nothing to check against")
    d = np.load(path)
    committed_sha = str(d["source_sha256"])
    if base.source_sha256() != committed_sha:
        print("the reference's datasets.py / utils.py changed: read the diff, then re-run this script")
        return False
    meth, _ = reference_methods(expect_sha256=committed_sha)
    again = compute(meth)
    y = {k: d[k] for k in d.files if k != "source_sha256"}
    bad = sorted(set(again) ^ set(y)) + [k for k in y if k in again and not (again[k].dtype == y[k].dtype and np.array_equal(again[k], y[k]))]
    print(f"{path}: " + ("equals what the reference computes, bit for bit" if not bad else "DIFFERS in " + ", ".join(bad[:10])))
    return not bad


if __name__ == "__main__":
    if sys.argv[1:] == ["--check"]:
        raise SystemExit(0 if check() else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
