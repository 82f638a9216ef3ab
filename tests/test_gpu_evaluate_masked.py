"""evaluate.evaluate(..., masks=, mask_mode=): the reference's MASK / CROP scores (metric/summary.py:91-92,177-205) on the example scene.
The scene set-up is that of tests/test_gpu_evaluate.py (copied: that file stays as it is), at 200 x 200 to keep the renders short.
The masked scores are the existing device metrics on the multiplied / cut images, so they are compared for equality."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

pytestmark = pytest.mark.gpu
F32 = np.float32
S, F, P = 64, 128, 12
H = W = 200
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def scene():
    import cases
    from samplenerfro_amd import evaluate, models, prng, synthetic as syn, utils as U
    img = np.load(os.path.join(ROOT, "tests", "golden", "example_image.npz"))["rgba_sum4"]
    pixels = np.ascontiguousarray((img[..., :3].astype(F32) / F32(1020.0))[::2, ::2])   # every second pixel of the 400 x 400 view
    _, _, counts = cases.load_example_obj()
    grid = cases.example_grid(counts).astype(F32)
    focal = 0.5 * W / math.tan(0.5 * cases.EXAMPLE_CAMERA_ANGLE_X)                    # datasets.py:361
    flags = U.default_flags(num_coarse_samples=S, num_fine_samples=F, num_path_samples=P, white_bkgd=False, use_online_sparsity=False,
                            randomized=True, near=2.0, far=6.0, batch_size=1024, bg_weight=0.025, bg_smooth_weight=1.0, bg_patch_size=128,
                            config="configs/example")
    seed = 3
    model, variables = models.construct_nerf(np.array([0, seed], np.uint32), None, flags, [128] * 3, [-1.5] * 3, [1.5] * 3, T(grid))
    pf = syn.init_params_flat(seed, fine=True)
    for k in ("coarse_mlp", "fine_mlp", "bkgd_mlp"):
        variables["flat"][k].copy_(T(pf[k]))
    rng = prng.PRNGKey(4)
    c2w = np.asarray(cases.EXAMPLE_C2W, F32)
    views = list(evaluate.device_views(np.stack([pixels] * 2), np.stack([c2w] * 2), focal=focal, device=torch.device(DEV)))
    fn = lambda k0, k1, r, path=None: model.apply(variables, k0, k1, r, False, path=path)
    rgb, _, _ = U.render_image(fn, views[0]["rays"], rng, False, chunk=8192, model=model)
    # view 0: a 0 / 255 uint8 numpy disc; view 1: a 0 / 1 float device rectangle
    yy, xx = np.mgrid[:H, :W]
    disc = (((yy - 90) ** 2 + (xx - 110) ** 2) < 55 ** 2).astype(np.uint8) * 255
    rect = torch.zeros((H, W), device=DEV)
    rect[30:150, 60:121] = 1.0
    return dict(model=model, variables=variables, rng=rng, views=views, rgb=rgb, masks=[disc, rect])


def run(scene, **kw):
    from samplenerfro_amd import evaluate
    return evaluate.evaluate(scene["model"], scene["variables"], iter(scene["views"]), scene["rng"], chunk=8192, **kw)


def by_hand(scene, idx, mode):
    """The three scores of view idx: summary.py:197-205 written out, then the metric calls of the unmasked loop."""
    from samplenerfro_amd import utils as U
    pred, pix, m = scene["rgb"], scene["views"][idx]["pixels"], scene["masks"][idx]
    m = (torch.as_tensor(m).to(DEV) > 0)
    if mode in ("mask", "mask_crop"):
        pred, pix = pred * m[..., None].float(), pix * m[..., None].float()
    if mode in ("crop", "mask_crop"):
        rows, cols = torch.nonzero(m.any(1))[:, 0], torch.nonzero(m.any(0))[:, 0]
        y0, y1, x0, x1 = int(rows.min()), int(rows.max()) + 1, int(cols.min()), int(cols.max()) + 1
        pred, pix = pred[y0:y1, x0:x1].contiguous(), pix[y0:y1, x0:x1].contiguous()
    vals = torch.stack([U.compute_psnr(((pred - pix) ** 2).mean()).to(torch.float32), U.compute_ssim(pred, pix, max_val=1.0),
                        U.compute_flip(pred, pix, None)]).cpu()
    return [float(v) for v in vals], tuple(pred.shape)


@pytest.mark.parametrize("mode,suffix", [("mask", "_mask"), ("crop", "_crop"), ("mask_crop", "_mask")])
def test_masked_scores_equal_the_metrics_on_the_masked_images(scene, tmp_path, mode, suffix):
    res = run(scene, masks=scene["masks"], mask_mode=mode, flip=True, out_dir=str(tmp_path), step=7, save_output=True)
    assert res["mask_mode"] == mode and len(res["psnrs"]) == 2
    shapes = []
    for idx in range(2):
        want, shape = by_hand(scene, idx, mode)
        shapes.append(shape)
        assert [res["psnrs"][idx], res["ssims"][idx], res["flips"][idx]] == want, (idx, mode)
    assert shapes == ([(H, W, 3)] * 2 if mode == "mask" else [(109, 109, 3), (120, 61, 3)])
    assert res["psnrs"][0] != res["psnrs"][1]                                          # the two masks score differently
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["000.png", "001.png", "disp_000.png", "disp_001.png"] +
                           [f"{n}{suffix}.txt" for n in ("psnr", "ssim", "flip", "psnrs_7", "ssims_7", "flips_7")])
    for key, stem in (("psnrs", "psnr"), ("ssims", "ssim"), ("flips", "flip")):
        vals = [float(v) for v in (tmp_path / f"{stem}s_7{suffix}.txt").read_text().split(" ")]
        assert vals == res[key] and float((tmp_path / f"{stem}{suffix}.txt").read_text()) == float(np.mean(np.array(vals)))
    from PIL import Image
    png = np.asarray(Image.open(tmp_path / "000.png"))
    assert png.shape == (H, W, 3) and png[scene["masks"][0] == 0].any()                # written unmasked: colour outside the mask too


def test_defaults_all_ones_mask_and_errors(scene):
    stable = lambda r: {k: v for k, v in r.items() if k not in ("seconds", "rays_per_sec")}
    plain = run(scene)
    assert sorted(plain) == ["psnr", "psnrs", "rays_per_sec", "seconds", "ssim", "ssims"]         # the keys of a call made before masks existed
    assert stable(run(scene, masks=None, mask_mode=None)) == stable(plain)
    ones = run(scene, masks=[np.ones((H, W), np.uint8)] * 2, mask_mode="mask")
    assert ones.pop("mask_mode") == "mask" and stable(ones) == stable(plain)           # x * 1.0 is x: exactly the unmasked scores
    want, _ = by_hand(scene, 0, None)
    assert [plain["psnrs"][0], plain["ssims"][0]] == want[:2]
    with pytest.raises(ValueError, match="go together"):
        run(scene, masks=scene["masks"])
    with pytest.raises(ValueError, match="go together"):
        run(scene, mask_mode="crop")
    with pytest.raises(ValueError, match="mask_mode must be one of"):
        run(scene, masks=scene["masks"], mask_mode="both")
    tiny = np.zeros((H, W), np.uint8); tiny[50:55, 40:80] = 1
    with pytest.raises(ValueError, match="5 pixels.*SSIM window|40 x 5"):
        run(scene, masks=[tiny, tiny], mask_mode="crop")
    with pytest.raises(ValueError, match="0 x 0"):
        run(scene, masks=[np.zeros((H, W), np.uint8)] * 2, mask_mode="mask_crop")
    with pytest.raises(ValueError, match="ran out"):
        run(scene, masks=scene["masks"][:1], mask_mode="mask")
