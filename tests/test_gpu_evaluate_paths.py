"""samplenerfro_amd.evaluate with path_maps=True on a 40 x 48 crop of the example scene's view: the three PNGs per view hold
paths.visualize_maps(paths.view_maps(...)) through utils.save_img, "refracted" is the restated fraction, it also works without ground
truth, and a run without the flag writes the files and returns the keys it always did."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import paths_ref as R               # noqa: E402
import paths_scene as PS            # noqa: E402

pytestmark = pytest.mark.gpu
MAP_NAMES = ("mask", "bend", "optical")


@pytest.fixture(scope="module")
def crop():
    return PS.example_crop()


def test_evaluate_writes_the_refraction_maps(crop, tmp_path):
    from PIL import Image
    from samplenerfro_amd import evaluate, paths, prng, utils as U
    model, variables = crop["model"], crop["variables"]
    rng = prng.PRNGKey(4)
    views = [{"rays": crop["rays"], "pixels": crop["pixels"]}]
    with_dir, without_dir, here = tmp_path / "with", tmp_path / "without", tmp_path / "here"
    res = evaluate.evaluate(model, variables, iter(views), rng, chunk=700, out_dir=str(with_dir), step=7, save_output=True, path_maps=True)
    plain = evaluate.evaluate(model, variables, iter(views), rng, chunk=700, out_dir=str(without_dir), step=7, save_output=True)

    maps = paths.view_maps(model, variables, crop["rays"], chunk=8192)
    vis = paths.visualize_maps(maps)
    os.makedirs(here)
    for name in MAP_NAMES:
        U.save_img(vis[name], str(here / f"{name}.png"))
        got = np.asarray(Image.open(with_dir / f"{name}_000.png"))
        assert got.shape == ((40, 48) if name == "mask" else (40, 48, 3)) and got.dtype == np.uint8
        assert np.array_equal(got, np.asarray(Image.open(here / f"{name}.png"))), name
    mask = np.asarray(Image.open(with_dir / "mask_000.png"))
    assert set(np.unique(mask).tolist()) == {0, 255}

    # the fraction, restated from the records of one whole march read back
    flat = U.Rays(crop["rays"].origins.reshape(-1, 3), None, crop["rays"].viewdirs.reshape(-1, 3), None)
    pd, dr, ior = (t.cpu().numpy() for t in paths.march(model, variables, flat))
    count = int((R.summary(pd, dr, ior)[0][0] > 0).sum())
    assert res["refracted"] == [count / (40 * 48)] and 0 < count < 40 * 48
    assert np.array_equal(mask.reshape(-1) == 255, R.refracting(ior).any(0))     # eval.py:173's pred_mask

    # the flag off: the files and the keys of the loop without it; with it, only the three PNGs per view and one key are new
    old = ["000.png", "disp_000.png", "psnr.txt", "psnrs_7.txt", "ssim.txt", "ssims_7.txt"]
    assert sorted(os.listdir(without_dir)) == old
    assert sorted(os.listdir(with_dir)) == sorted(old + [f"{n}_000.png" for n in MAP_NAMES])
    for name in old:
        assert (with_dir / name).read_bytes() == (without_dir / name).read_bytes(), name
    assert sorted(plain) == ["psnr", "psnrs", "rays_per_sec", "seconds", "ssim", "ssims"] and sorted(res) == sorted(list(plain) + ["refracted"])
    assert plain["psnrs"] == res["psnrs"] and plain["ssims"] == res["ssims"]


def test_path_maps_with_render_path(crop, tmp_path):
    from samplenerfro_amd import evaluate, prng
    views = [{"rays": crop["rays"], "pixels": crop["pixels"]}] * 2
    res = evaluate.evaluate(crop["model"], crop["variables"], iter(views), prng.PRNGKey(4), out_dir=str(tmp_path), step=7, render_path=True,
                            save_output=True, path_maps=True)
    assert res["psnrs"] == [] and len(res["refracted"]) == 2 and res["refracted"][0] == res["refracted"][1]
    assert sorted(os.listdir(tmp_path)) == sorted([f"{i:03d}.png" for i in range(2)] + [f"disp_{i:03d}.png" for i in range(2)] +
                                                  [f"{n}_{i:03d}.png" for n in MAP_NAMES for i in range(2)])
    before = {n: (tmp_path / n).stat().st_mtime_ns for n in os.listdir(tmp_path)}
    quiet = evaluate.evaluate(crop["model"], crop["variables"], iter(views[:1]), prng.PRNGKey(4), out_dir=str(tmp_path), render_path=True,
                              path_maps=True)                                    # without save_output nothing is written
    assert quiet["refracted"] == res["refracted"][:1]
    assert {n: (tmp_path / n).stat().st_mtime_ns for n in os.listdir(tmp_path)} == before
