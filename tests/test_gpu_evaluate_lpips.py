"""samplenerfro_amd.evaluate with lpips=weights on the example scene (the set-up of tests/test_gpu_evaluate_errmap.py at 64 x 64, one
view, seeded random LPIPS weights): the keys and the metric files, with errmap=True the six-panel sheet whose third map is the coloured,
clipped LPIPS map, lpips_000.png and the four-column texts; a crop below 31 x 31 is refused by name; lpips=None changes nothing."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import errmap_ref as E              # noqa: E402
import lpips_ref as R               # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
S, F, P = 64, 128, 12
H = W = 64
DEV = "cuda:0"
OLD = ["000.png", "disp_000.png", "psnr.txt", "psnrs_7.txt", "ssim.txt", "ssims_7.txt"]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def scene():
    import cases
    from samplenerfro_amd import evaluate, lpips, models, prng, synthetic as syn, utils as U
    img = np.load(os.path.join(ROOT, "tests", "golden", "example_image.npz"))["rgba_sum4"]
    pixels = np.ascontiguousarray((img[..., :3].astype(F32) / F32(1020.0))[8::6, 8::6][:H, :W])
    _, _, counts = cases.load_example_obj()
    grid = cases.example_grid(counts).astype(F32)
    focal = 0.5 * W / math.tan(0.5 * cases.EXAMPLE_CAMERA_ANGLE_X)
    flags = U.default_flags(num_coarse_samples=S, num_fine_samples=F, num_path_samples=P, white_bkgd=False, use_online_sparsity=False,
                            randomized=True, near=2.0, far=6.0, batch_size=1024, bg_weight=0.025, bg_smooth_weight=1.0, bg_patch_size=128,
                            config="configs/example")
    seed = 3
    model, variables = models.construct_nerf(np.array([0, seed], np.uint32), None, flags, [128] * 3, [-1.5] * 3, [1.5] * 3, T(grid))
    pf = syn.init_params_flat(seed, fine=True)
    for k in ("coarse_mlp", "fine_mlp", "bkgd_mlp"):
        variables["flat"][k].copy_(T(pf[k]))
    rng = prng.PRNGKey(4)
    views = list(evaluate.device_views(pixels[None], np.asarray(cases.EXAMPLE_C2W, F32)[None], focal=focal, device=torch.device(DEV)))
    fn = lambda k0, k1, r, path=None: model.apply(variables, k0, k1, r, False, path=path)
    rgb, _, _ = U.render_image(fn, views[0]["rays"], rng, False, chunk=8192, model=model)
    w = R.weight_set()
    weights = lpips.from_tensors(w["convs"], w["biases"], w["lins"], device=DEV)
    return dict(model=model, variables=variables, rng=rng, views=views, pixels=pixels, rgb=rgb.cpu().numpy(), weights=weights)


def run(scene, **kw):
    from samplenerfro_amd import evaluate
    return evaluate.evaluate(scene["model"], scene["variables"], iter(scene["views"]), scene["rng"], chunk=8192, step=7, **kw)


def tree(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs)


def test_lpips_none_changes_nothing(scene, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    plain = run(scene, out_dir=str(a), save_output=True, errmap=True)
    none = run(scene, out_dir=str(b), save_output=True, errmap=True, lpips=None)
    assert sorted(plain) == sorted(none) and sorted(plain["summary"]) == sorted(none["summary"])
    assert tree(a) == tree(b) and "errmap/lpips_000.png" not in tree(a)
    for name in tree(a):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    assert {k: v for k, v in plain.items() if k not in ("seconds", "rays_per_sec")} == {k: v for k, v in none.items() if k not in ("seconds", "rays_per_sec")}


def test_evaluate_scores_lpips_and_writes_its_files(scene, tmp_path):
    from samplenerfro_amd import utils
    res = run(scene, out_dir=str(tmp_path), save_output=True, lpips=scene["weights"])
    assert sorted(res) == ["lpips", "lpips_values", "psnr", "psnrs", "rays_per_sec", "seconds", "ssim", "ssims"]
    assert tree(tmp_path) == sorted(OLD + ["lpips.txt", "lpips_7.txt"])
    want = float(utils.compute_lpips(scene["pixels"], scene["rgb"], scene["weights"]).cpu())
    assert res["lpips_values"] == [want] and res["lpips"] == want and 0.0 < want < 4.0
    assert (tmp_path / "lpips_7.txt").read_text() == str(want) and (tmp_path / "lpips.txt").read_text() == "{}".format(np.mean(np.array([want])))
    both = run(scene, flip=True, lpips=scene["weights"])                      # the floats share the read-back with FLIP's
    assert both["lpips_values"] == [want] and len(both["flips"]) == 1 and both["psnrs"] == res["psnrs"]


def test_errmap_with_lpips_gives_the_six_panel_sheet(scene, tmp_path):
    from PIL import Image
    from samplenerfro_amd import errmap
    res = run(scene, out_dir=str(tmp_path), save_output=True, errmap=True, lpips=scene["weights"])
    new = ["errmap/flip_000.png", "errmap/frame/frame_000.png", "errmap/lpips_000.png", "errmap/psnr_000.png", "errmap/ssim_000.png",
           "lpips.txt", "lpips_7.txt", "metric_list.txt", "result.txt"]
    assert tree(tmp_path) == sorted(OLD + new)
    assert sorted(res) == ["lpips", "lpips_values", "psnr", "psnrs", "rays_per_sec", "seconds", "ssim", "ssims", "summary"]
    s = res["summary"]
    assert sorted(s) == ["flip", "flips", "lpips", "lpips_values", "psnr", "psnrs", "ssim", "ssims"]

    # what errmap.error_maps makes of the ground truth and the 8-bit render, called directly
    q = E.quantize8(scene["rgb"])
    maps = errmap.error_maps(T(scene["pixels"]), T(q), lpips=scene["weights"])
    names = errmap.MAP_NAMES_LPIPS
    host = [maps[n].cpu().numpy() for n in names]
    values = [float(maps[n + "_value"].cpu()) for n in names]
    assert [m.shape for m in host] == [(H, W), (H - 10, W - 10), (H, W), (H, W)]
    raw_map, raw_value = utils_lpips_both(scene, q)
    assert np.array_equal(host[2], np.clip(raw_map, 0.0, 1.0)) and values[2] == raw_value
    assert [s["psnrs"], s["ssims"], s["lpips_values"], s["flips"]] == [[v] for v in values]
    assert [s["psnr"], s["ssim"], s["lpips"], s["flip"]] == values
    assert s["lpips_values"] != res["lpips_values"]                           # the 8-bit image: another number than the float render's

    want_sheet = E.sheet(scene["pixels"], q, host)
    assert want_sheet.shape == (H, 6 * (W + 5), 3)
    got_sheet = np.asarray(Image.open(tmp_path / "errmap" / "frame" / "frame_000.png"))
    assert got_sheet.dtype == np.uint8 and got_sheet.shape == (H, 6 * (W + 5), 3) and np.array_equal(got_sheet, want_sheet)
    third = got_sheet[:, 4 * (W + 5):4 * (W + 5) + W]
    assert np.array_equal(third, errmap.colorize(T(np.clip(raw_map, 0.0, 1.0))).cpu().numpy()) and third.reshape(-1, 3).any(0).all()
    for k, (name, m) in enumerate(zip(names, host)):
        x0 = (2 + k) * (W + 5)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "errmap" / f"{name}_000.png")), want_sheet[:m.shape[0], x0:x0 + m.shape[1]]), name
    assert (tmp_path / "metric_list.txt").read_text() == f"{0:3d}{values[0]:6.2f}{values[1]:6.3f}{values[2]:6.3f}{values[3]:6.3f}\n"
    assert (tmp_path / "result.txt").read_text() == f"{values[0]:6.2f}{values[1]:6.3f}{values[2]:6.3f}{values[3]:6.3f}\n"


def utils_lpips_both(scene, q):
    from samplenerfro_amd import ops
    m, v = ops.lpips(T(scene["pixels"]), T(q), scene["weights"], return_both=True)
    return m.cpu().numpy(), float(v.cpu())


def test_a_crop_below_31_pixels_is_refused_by_name(scene):
    mask = np.zeros((H, W), np.uint8)
    mask[10:30, 20:40] = 255                                                 # 20 x 20: enough for SSIM, not for LPIPS
    run(scene, masks=[mask], mask_mode="crop")
    with pytest.raises(ValueError, match="LPIPS"):
        run(scene, masks=[mask], mask_mode="crop", lpips=scene["weights"])
    with pytest.raises(ValueError, match="LPIPS"):
        run(scene, masks=[mask], mask_mode="mask_crop", errmap=True, lpips=scene["weights"])
    mask[10:45, 20:51] = 255                                                 # 35 x 31: the smallest LPIPS takes
    res = run(scene, masks=[mask], mask_mode="crop", errmap=True, lpips=scene["weights"])
    assert len(res["lpips_values"]) == 1 and len(res["summary"]["lpips_values"]) == 1
