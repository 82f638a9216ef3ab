"""samplenerfro_amd.evaluate with flip=True on the example scene (the set-up of tests/test_gpu_evaluate.py): the FLIP values are those of
utils.compute_flip on the same rendered frame, the extra files hold them, and PSNR / SSIM and their files are bit-equal to a run without
FLIP, which has neither the keys nor the files."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import flip_ref                      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
S, F, P = 64, 128, 12


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


def test_evaluate_scores_flip_beside_psnr_and_ssim(scene, tmp_path):
    from samplenerfro_amd import evaluate, prng, utils as U
    dev = torch.device("cuda:0")
    model, variables = scene["model"], scene["variables"]
    rng = prng.PRNGKey(4)
    images, c2ws = np.stack([scene["pixels"]] * 2), np.stack([scene["c2w"]] * 2)
    views = list(evaluate.device_views(images, c2ws, focal=scene["focal"], device=dev))
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    ppd = U.FLIP_PPD_SUMMARY
    res = evaluate.evaluate(model, variables, iter(views), rng, chunk=8192, out_dir=str(with_dir), step=7, save_output=True, flip=True,
                            flip_pixels_per_degree=ppd)
    plain = evaluate.evaluate(model, variables, iter(views), rng, chunk=8192, out_dir=str(without_dir), step=7, save_output=True)

    # the same frame rendered here, scored by compute_flip: the same bits
    fn = lambda k0, k1, r, path=None: model.apply(variables, k0, k1, r, False, path=path)
    rgb, _, _ = U.render_image(fn, views[0]["rays"], rng, False, chunk=8192, model=model)
    want = float(U.compute_flip(rgb, views[0]["pixels"], ppd))
    assert res["flips"] == [want, want] and res["flip"] == float(np.mean(np.array(res["flips"])))
    # and that value is LDR-FLIP of the frame against the photograph: the float32 rule on a mean
    frame = rgb.cpu().numpy()
    m64, m32 = flip_ref.flip(frame, scene["pixels"], ppd), flip_ref.flip(frame, scene["pixels"], ppd, dtype=np.float32)
    bound = 2 * float(np.mean(np.abs(m32 - m64))) + 1e-6
    print(f"example view: FLIP {want:.6f} (float64 {np.mean(m64):.6f}, bound {bound:.3g}) at {ppd:.4g} ppd")
    assert abs(want - float(np.mean(m64))) <= bound
    # the default pixels_per_degree is compute_ldrflip's
    res_default = evaluate.evaluate(model, variables, iter(views[:1]), rng, chunk=8192, flip=True)
    assert res_default["flips"] == [float(U.compute_flip(rgb, views[0]["pixels"]))] and res_default["flips"][0] != want

    # files: the two new ones hold the values; the others are byte-equal to the run without FLIP
    assert sorted(os.listdir(with_dir)) == ["000.png", "001.png", "disp_000.png", "disp_001.png", "flip.txt", "flips_7.txt", "psnr.txt",
                                            "psnrs_7.txt", "ssim.txt", "ssims_7.txt"]
    assert [float(v) for v in (with_dir / "flips_7.txt").read_text().split(" ")] == res["flips"]
    assert float((with_dir / "flip.txt").read_text()) == res["flip"]
    names = sorted(os.listdir(without_dir))
    assert names == ["000.png", "001.png", "disp_000.png", "disp_001.png", "psnr.txt", "psnrs_7.txt", "ssim.txt", "ssims_7.txt"]
    for name in names:
        assert (with_dir / name).read_bytes() == (without_dir / name).read_bytes(), name
    assert "flips" not in plain and "flip" not in plain
    assert sorted(plain) == ["psnr", "psnrs", "rays_per_sec", "seconds", "ssim", "ssims"]
    assert plain["psnrs"] == res["psnrs"] and plain["ssims"] == res["ssims"] and plain["psnr"] == res["psnr"] and plain["ssim"] == res["ssim"]


def test_render_path_with_flip_has_no_values(scene, tmp_path):
    from samplenerfro_amd import evaluate, prng
    views = evaluate.device_views(scene["pixels"][None], scene["c2w"][None], focal=scene["focal"], device=torch.device("cuda:0"))
    res = evaluate.evaluate(scene["model"], scene["variables"], views, prng.PRNGKey(4), out_dir=str(tmp_path), step=7, save_output=True,
                            render_path=True, flip=True)
    assert res["flips"] == [] and res["flip"] is None
    assert sorted(os.listdir(tmp_path)) == ["000.png", "disp_000.png"]
