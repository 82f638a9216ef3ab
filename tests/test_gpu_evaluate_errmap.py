"""samplenerfro_amd.evaluate with errmap=True on the example scene (the set-up of tests/test_gpu_evaluate_vis.py at 64 x 64, one view):
the files of metric/summary.py hold what tests/helpers/errmap_ref.py makes of the read-back render, the ground truth and the device's
maps; the summary numbers are errmap.error_maps' own; a run without the flag writes the files and returns the keys it always did."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import errmap_ref as R               # noqa: E402

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
    from samplenerfro_amd import evaluate, models, prng, synthetic as syn, utils as U
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
    return dict(model=model, variables=variables, rng=rng, views=views, pixels=pixels, rgb=rgb.cpu().numpy())


def run(scene, **kw):
    from samplenerfro_amd import evaluate
    return evaluate.evaluate(scene["model"], scene["variables"], iter(scene["views"]), scene["rng"], chunk=8192, step=7, **kw)


def tree(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs)


def expected(pixels, pred):
    """(the helper's sheet, the maps' shapes, error_maps called directly) for ground truth and the read-back float render, both numpy."""
    from samplenerfro_amd import errmap
    q = R.quantize8(pred)
    maps = errmap.error_maps(T(pixels), T(q))
    host = [maps[n].cpu().numpy() for n in errmap.MAP_NAMES]
    return R.sheet(pixels, q, host), [m.shape for m in host], [float(maps[n + "_value"].cpu()) for n in errmap.MAP_NAMES]


def test_evaluate_writes_summarys_files(scene, tmp_path):
    from PIL import Image
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    res = run(scene, out_dir=str(with_dir), save_output=True, errmap=True)
    plain = run(scene, out_dir=str(without_dir), save_output=True)

    # the flag off: the files and the keys of the loop without it; with it, only summary.py's files and the "summary" key are new
    assert tree(without_dir) == OLD
    new = ["errmap/flip_000.png", "errmap/frame/frame_000.png", "errmap/psnr_000.png", "errmap/ssim_000.png", "metric_list.txt", "result.txt"]
    assert tree(with_dir) == sorted(OLD + new)
    for name in OLD:
        assert (with_dir / name).read_bytes() == (without_dir / name).read_bytes(), name
    assert sorted(plain) == ["psnr", "psnrs", "rays_per_sec", "seconds", "ssim", "ssims"] and sorted(res) == sorted(list(plain) + ["summary"])
    assert plain["psnrs"] == res["psnrs"] and plain["ssims"] == res["ssims"]

    want_sheet, shapes, values = expected(scene["pixels"], scene["rgb"])
    assert shapes == [(H, W), (H - 10, W - 10), (H, W)] and want_sheet.shape == (H, 5 * (W + 5), 3)
    got_sheet = np.asarray(Image.open(with_dir / "errmap" / "frame" / "frame_000.png"))
    assert got_sheet.dtype == np.uint8 and np.array_equal(got_sheet, want_sheet)
    for k, (name, (h, w)) in enumerate(zip(("psnr", "ssim", "flip"), shapes)):
        x0 = (2 + k) * (W + 5)
        assert np.array_equal(np.asarray(Image.open(with_dir / "errmap" / f"{name}_000.png")), want_sheet[:h, x0:x0 + w]), name
    assert want_sheet[:, 2 * (W + 5):].reshape(-1, 3).any(0).all()       # the panels are not empty
    s = res["summary"]
    assert sorted(s) == ["flip", "flips", "psnr", "psnrs", "ssim", "ssims"]
    assert [s["psnrs"], s["ssims"], s["flips"]] == [[v] for v in values] and [s["psnr"], s["ssim"], s["flip"]] == values
    assert (with_dir / "metric_list.txt").read_text() == f"{0:3d}{values[0]:6.2f}{values[1]:6.3f}{values[2]:6.3f}\n"
    assert (with_dir / "result.txt").read_text() == f"{values[0]:6.2f}{values[1]:6.3f}{values[2]:6.3f}\n"
    assert s["psnrs"] != res["psnrs"] and s["ssims"] != res["ssims"]      # the 8-bit image under another SSIM: other numbers

    quiet = run(scene, errmap=True)                                      # without save_output: the numbers, no files
    assert quiet["summary"] == s
    with pytest.raises(ValueError, match="render_path"):
        run(scene, errmap=True, render_path=True)


@pytest.mark.parametrize("mode,suffix", [("crop", "_crop"), ("mask_crop", "_mask")])
def test_a_cropped_view_gives_a_cropped_sheet(scene, tmp_path, mode, suffix):
    from PIL import Image
    mask = np.zeros((H, W), np.uint8)
    mask[10:45, 20:51] = 255                                             # 35 rows x 31 columns
    res = run(scene, out_dir=str(tmp_path), save_output=True, errmap=True, masks=[mask], mask_mode=mode)
    new = [f"errmap{suffix}/flip_000.png", f"errmap{suffix}/frame{suffix}/frame_000.png", f"errmap{suffix}/psnr_000.png", f"errmap{suffix}/ssim_000.png",
           f"metric_list{suffix}.txt", f"result{suffix}.txt"]
    assert tree(tmp_path) == sorted(["000.png", "disp_000.png"] + [f"{n}{suffix}.txt" for n in ("psnr", "psnrs_7", "ssim", "ssims_7")] + new)
    m = (mask > 0).astype(F32)[..., None] if mode == "mask_crop" else F32(1)
    pixels, pred = (scene["pixels"] * m)[10:45, 20:51], (scene["rgb"] * m)[10:45, 20:51]
    want_sheet, shapes, values = expected(pixels, pred)
    assert shapes == [(35, 31), (25, 21), (35, 31)]
    got = np.asarray(Image.open(tmp_path / f"errmap{suffix}" / f"frame{suffix}" / "frame_000.png"))
    assert got.shape == (35, 5 * 36, 3) and np.array_equal(got, want_sheet)
    assert np.asarray(Image.open(tmp_path / f"errmap{suffix}" / "ssim_000.png")).shape == (25, 21, 3)
    assert [res["summary"]["psnr"], res["summary"]["ssim"], res["summary"]["flip"]] == values and res["mask_mode"] == mode
