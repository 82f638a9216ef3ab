"""samplenerfro_amd.evaluate with vis_suite=True on the example scene (the set-up of tests/test_gpu_evaluate.py, one view): the three
depth PNGs of eval.py:196-198 per view hold what vis.visualize_suite gives for the same rendered disp / acc through utils.save_img, and
a run without the flag writes the files and returns the keys it always did."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

pytestmark = pytest.mark.gpu
F32 = np.float32
S, F, P = 64, 128, 12
VIS_NAMES = ("depth", "depth_mod", "depth_normals")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def scene():
    import cases
    from samplenerfro_amd import models, synthetic as syn, utils as U
    img = np.load(os.path.join(ROOT, "tests", "golden", "example_image.npz"))["rgba_sum4"]
    pixels = (img[..., :3].astype(F32) / F32(1020.0))
    _, _, counts = cases.load_example_obj()
    grid = cases.example_grid(counts).astype(F32)
    H = W = 400
    focal = 0.5 * W / math.tan(0.5 * cases.EXAMPLE_CAMERA_ANGLE_X)
    flags = U.default_flags(num_coarse_samples=S, num_fine_samples=F, num_path_samples=P, white_bkgd=False, use_online_sparsity=False,
                            randomized=True, near=2.0, far=6.0, batch_size=1024, bg_weight=0.025, bg_smooth_weight=1.0, bg_patch_size=128,
                            config="configs/example")
    seed = 3
    model, variables = models.construct_nerf(np.array([0, seed], np.uint32), None, flags, [128] * 3, [-1.5] * 3, [1.5] * 3, T(grid))
    pf = syn.init_params_flat(seed, fine=True)
    for k in ("coarse_mlp", "fine_mlp", "bkgd_mlp"):
        variables["flat"][k].copy_(T(pf[k]))
    return dict(pixels=pixels, H=H, W=W, focal=focal, c2w=np.asarray(cases.EXAMPLE_C2W, F32), model=model, variables=variables)


def test_evaluate_writes_the_depth_visualisations(scene, tmp_path):
    from PIL import Image
    from samplenerfro_amd import evaluate, prng, utils as U, vis
    dev = torch.device("cuda:0")
    model, variables = scene["model"], scene["variables"]
    rng = prng.PRNGKey(4)
    views = list(evaluate.device_views(scene["pixels"][None], scene["c2w"][None], focal=scene["focal"], device=dev))
    with_dir, without_dir, here = tmp_path / "with", tmp_path / "without", tmp_path / "here"
    res = evaluate.evaluate(model, variables, iter(views), rng, chunk=8192, out_dir=str(with_dir), step=7, save_output=True, vis_suite=True)
    plain = evaluate.evaluate(model, variables, iter(views), rng, chunk=8192, out_dir=str(without_dir), step=7, save_output=True)

    # the same frame rendered here: the suite of its disp / acc, through save_img
    fn = lambda k0, k1, r, path=None: model.apply(variables, k0, k1, r, False, path=path)
    _, disp, acc = U.render_image(fn, views[0]["rays"], rng, False, chunk=8192, model=model)
    suite = vis.visualize_suite(disp[..., 0], acc[..., 0])
    os.makedirs(here)
    for name in VIS_NAMES:
        U.save_img(suite[name], str(here / f"{name}.png"))
        got = np.asarray(Image.open(with_dir / f"{name}_000.png"))
        assert got.shape == (scene["H"], scene["W"], 3) and got.dtype == np.uint8
        assert np.array_equal(got, np.asarray(Image.open(here / f"{name}.png"))), name
        assert np.array_equal(got, (np.clip(suite[name].cpu().numpy(), 0.0, 1.0) * 255.0).astype(np.uint8)), name

    # the flag off: the files and the keys of the loop without it; with it, only the three PNGs per view are new
    old = ["000.png", "disp_000.png", "psnr.txt", "psnrs_7.txt", "ssim.txt", "ssims_7.txt"]
    assert sorted(os.listdir(without_dir)) == old
    assert sorted(os.listdir(with_dir)) == sorted(old + [f"{n}_000.png" for n in VIS_NAMES])
    for name in old:
        assert (with_dir / name).read_bytes() == (without_dir / name).read_bytes(), name
    assert sorted(plain) == ["psnr", "psnrs", "rays_per_sec", "seconds", "ssim", "ssims"] and sorted(res) == sorted(plain)
    assert plain["psnrs"] == res["psnrs"] and plain["ssims"] == res["ssims"]


def test_vis_suite_without_save_output_writes_nothing(scene, tmp_path):
    from samplenerfro_amd import evaluate, prng
    views = evaluate.device_views(scene["pixels"][None], scene["c2w"][None], focal=scene["focal"], device=torch.device("cuda:0"))
    res = evaluate.evaluate(scene["model"], scene["variables"], views, prng.PRNGKey(4), out_dir=str(tmp_path), step=7, render_path=True,
                            vis_suite=True)
    assert res["psnrs"] == [] and os.listdir(tmp_path) == []
