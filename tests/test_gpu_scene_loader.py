"""rnerf_images_prepare and samplenerfro_amd.datasets' scene loaders on the device.  Every comparison is bit for bit: against the numpy
float32 definition (tests/helpers/scene_fixture.prepare_reference), against what the reference's own loaders computed on the same tiny
scenes at `factor: 0` (tests/golden/scene_loader_reference.npz), against ops.generate_rays for the rays, and against a DeviceBatcher
built by hand for the train split.  `factor: 2` is checked against the definition (the reference needs cv2 there; the stated deviation
is tests/test_scene_loader_host.py's)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import scene_fixture as SF      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "scene_loader_reference.npz"))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    import make_scene_loader_reference as M
    return M.write_scenes(str(tmp_path_factory.mktemp("scenes")))


def flags_of(dataset, data_dir, **over):
    from samplenerfro_amd import utils
    return utils.default_flags(**dict(dict(dataset=dataset, data_dir=data_dir, factor=0, white_bkgd=False), **over))


def same(t, a):
    got = t.cpu().numpy()
    return got.dtype == a.dtype and got.shape == a.shape and np.array_equal(got, a)


PREPARE_CASES = [(shape, C, factor, white) for shape in ((2, 6, 10), (1, 2, 2), (3, 66, 130)) for C in (3, 4) for factor in (1, 2)
                 for white in ((0, 1) if C == 4 else (0,))]


@pytest.mark.parametrize("shape,C,factor,white", PREPARE_CASES)
def test_images_prepare_equals_the_definition(shape, C, factor, white):
    """(3, 66, 130) is more than one 256-thread block with a grid tail at either factor; widths 10 and 130 are multiples of no vector
    width; (1, 2, 2) is one output pixel at factor 2.  The all-0 and the all-255 image ride along as two more views."""
    from samplenerfro_amd import ops
    n, H, W = shape
    rng = np.random.default_rng(1000 * H + 10 * C + factor)
    u8 = np.concatenate([rng.integers(0, 256, (n, H, W, C), dtype=np.uint8), np.zeros((1, H, W, C), np.uint8), np.full((1, H, W, C), 255, np.uint8)])
    if C == 4:
        u8[0, : H // 2, : W // 2, 3] = 0                   # whole transparent and whole opaque 2 x 2 cells among the random alphas
        u8[0, H // 2:, W // 2:, 3] = 255
    want = SF.prepare_reference(u8, factor, bool(white))
    got = ops.images_prepare(torch.from_numpy(u8).to(DEV), factor, bool(white))
    assert same(got, want)
    assert np.all(want[-1] == 1.0) and np.all(want[-2] == (1.0 if white else 0.0))
    out = torch.full((n + 2, H // factor, W // factor, 3), -7.0, device=DEV)
    assert ops.images_prepare(torch.from_numpy(u8).to(DEV), factor, bool(white), out=out) is out and same(out, want)


def test_images_prepare_refuses_what_it_cannot_do():
    from samplenerfro_amd import _lib, ops
    u8 = torch.zeros((1, 6, 10, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.RnerfError, match="white_bkgd needs"):
        ops.images_prepare(u8, 1, True)
    with pytest.raises(_lib.RnerfError, match="factor"):
        ops.images_prepare(u8, 4)
    with pytest.raises(_lib.RnerfError, match="even"):
        ops.images_prepare(torch.zeros((1, 5, 10, 3), dtype=torch.uint8, device=DEV), 2)
    with pytest.raises(_lib.RnerfError, match="dtype"):
        ops.images_prepare(u8.float())
    with pytest.raises(_lib.RnerfError, match="CUDA"):
        ops.images_prepare(u8.cpu())


LOADER_CASES = {"blender_test": ("blender", "blender", {}), "blender_test_white": ("blender", "blender", dict(white_bkgd=True)),
                "opencv_test": ("opencv", "opencv", {}), "opencv_test_white": ("opencv", "opencv", dict(white_bkgd=True)),
                "opencv_rgb_test": ("opencv_rgb", "opencv", {}), "blender_test_eval_train": ("blender", "blender", dict(eval_train=True)),
                "nsvf_test": ("nsvf", "nsvf", {}), "nsvf_test_white": ("nsvf", "nsvf", dict(white_bkgd=True))}


@pytest.mark.parametrize("case", sorted(LOADER_CASES))
def test_factor_0_test_splits_equal_the_references(case, ref, scenes):
    """images, camtoworlds and the camera against the reference's loader; every view's rays against ops.generate_rays for its camera;
    order and wrap-around over size + 1 calls; peek() does not advance."""
    from samplenerfro_amd import datasets, ops
    scene, dataset, over = LOADER_CASES[case]
    ds = datasets.get_dataset("test", flags_of(dataset, scenes[scene], **over), device=DEV)
    assert type(ds).__name__ == {"blender": "Blender", "opencv": "OpenCV", "nsvf": "NSVF"}[dataset]
    want = ref[f"{case}_images"]
    n = int(ref[f"{case}_n_examples"])
    assert ds.size == n == want.shape[0] and (ds.h, ds.w) == (int(ref[f"{case}_h"]), int(ref[f"{case}_w"]))
    assert same(ds.images, want)
    assert np.array_equal(ds.camtoworlds, ref[f"{case}_camtoworlds"])
    if dataset == "opencv":
        cam = dict(cam_mat=[[float(v) for v in row] for row in ref[f"{case}_cam_mat"]])
        assert ds.cam_mat == cam["cam_mat"] and ds.focal is None
    else:
        cam = dict(focal=float(ref[f"{case}_focal"]))
        assert ds.focal == cam["focal"] and ds.cam_mat is None
    first = ds.peek()
    assert ds.peek() is first and ds.test_it == 1
    for call in range(n + 1):
        b = next(ds)
        if call == 0:
            assert b is first
        i = call % n
        assert same(b["pixels"], want[i])
        o, _, v = ops.generate_rays(ref[f"{case}_camtoworlds"][i], ds.h, ds.w, DEV, pixel_center=False, **cam)
        assert torch.equal(b["rays"].origins, o) and torch.equal(b["rays"].viewdirs, v)
        assert b["rays"].directions is None and b["rays"].radii is None and tuple(o.shape) == (ds.h, ds.w, 3)


@pytest.mark.parametrize("name,precrop_iters", [("opencv_crop_off", 0), ("opencv_crop_on", 2)])
def test_the_opencv_test_crop(name, precrop_iters, ref, scenes):
    """OpenCV._next_test: pixels and rays of the central window, with precrop_iters (the half sides times precrop_frac) and without."""
    from samplenerfro_amd import datasets
    ds = datasets.get_dataset("test", flags_of("opencv", scenes["opencv"], precrop_iters=precrop_iters, precrop_frac=0.5), device=DEV)
    shapes = set()
    for call in range(ds.size + 1):
        b = next(ds)
        pix = ref[f"{name}_{call}_pixels"]
        shapes.add(pix.shape)
        assert same(b["pixels"], pix)
        assert tuple(b["rays"].origins.shape) == tuple(b["rays"].viewdirs.shape) == pix.shape
        assert same(b["rays"].origins, ref[f"{name}_{call}_origins"]) and same(b["rays"].viewdirs, ref[f"{name}_{call}_viewdirs"])
        assert b["pixels"].is_contiguous() and b["rays"].origins.is_contiguous()
    assert shapes == ({(4, 6, 3)} if precrop_iters else {(SF.H, SF.W, 3)})


@pytest.mark.parametrize("white", [False, True])
def test_blender_at_factor_2(white, tmp_path):
    from samplenerfro_amd import datasets
    wrote = SF.write_blender(str(tmp_path))
    for split in ("train", "test"):
        ds = datasets.get_dataset(split, flags_of("blender", str(tmp_path), factor=2, white_bkgd=white, batch_size=8), device=DEV, prefetch=0)
        assert same(ds.images, SF.prepare_reference(wrote[split], 2, white))
        assert (ds.h, ds.w, ds.size) == (SF.H // 2, SF.W // 2, SF.SPLITS[split])
        assert ds.focal == .5 * (SF.W // 2) / np.tan(.5 * SF.CAMERA_ANGLE_X)
    b = next(ds)
    assert same(b["pixels"], SF.prepare_reference(wrote["test"], 2, white)[0]) and tuple(b["rays"].origins.shape) == (SF.H // 2, SF.W // 2, 3)


def test_the_example_window_loads_to_the_example_image_fixture(tmp_path):
    """A one-frame Blender scene written from example_scene.npz's window, loaded with the example config's `factor: 2`, is rgba_sum4 / 1020
    of the matching block of example_image.npz — the array tests/test_gpu_example_scene.py trains on."""
    import json
    from PIL import Image
    from samplenerfro_amd import datasets
    ex = np.load(os.path.join(GOLDEN, "example_scene.npz"))
    r, c = (int(v) for v in ex["origin"])
    os.makedirs(tmp_path / "imgs")
    Image.fromarray(ex["window"]).save(str(tmp_path / "imgs" / "r_0.png"), "PNG")
    with open(tmp_path / "transforms_train.json", "w") as fp:
        json.dump({"camera_angle_x": float(ex["camera_angle_x"]), "frames": [{"file_path": "./imgs/r_0", "transform_matrix": ex["transform_matrix"].tolist()}]}, fp)
    ds = datasets.get_dataset("test", flags_of("blender", str(tmp_path), factor=2, eval_train=True), device=DEV)
    s4 = np.load(os.path.join(GOLDEN, "example_image.npz"))["rgba_sum4"][r // 2:r // 2 + 32, c // 2:c // 2 + 48]
    assert same(ds.images, (s4[..., :3].astype(F32) / F32(1020.0))[None])
    assert np.array_equal(ds.camtoworlds[0], ex["transform_matrix"].astype(F32)) and ds.focal == .5 * 48 / np.tan(.5 * float(ex["camera_angle_x"]))


def test_the_train_split_is_a_device_batcher_built_from_the_flags(scenes, ref):
    """Three next() calls with RandomState(7) equal, in pixels and rays, those of a DeviceBatcher built by hand from the same images,
    camtoworlds and camera.  precrop_iters = 2 of the 3: both crop branches are drawn; precrop_frac 0.75 leaves a 6 x 8 window, room for
    the 4 x 4 patch (at 0.5 the window is 4 x 6 and the reference's own randint(0, 0) raises)."""
    from samplenerfro_amd import datasets
    from samplenerfro_amd.datasets import DeviceBatcher
    for dataset, case in (("blender", "blender_test_eval_train"), ("opencv", "opencv_test_eval_train")):
        flags = flags_of(dataset, scenes[dataset], batch_size=16, bg_patch_size=4, precrop_iters=2, precrop_frac=0.75, use_pixel_centers=True)
        ds = datasets.get_dataset("train", flags, device=DEV, rng=np.random.RandomState(7), prefetch=0)
        assert isinstance(ds.batcher, DeviceBatcher) and ds.size == 3
        cam = dict(cam_mat=ds.cam_mat) if dataset == "opencv" else dict(focal=float(ref[f"{case}_focal"]))
        hand = DeviceBatcher(torch.from_numpy(ref[f"{case}_images"]).to(DEV), ref[f"{case}_camtoworlds"], batch_size=16, device=DEV, pixel_center=True,
                             batching="single_image", patch_size=4, precrop_iters=2, precrop_frac=0.75, rng=np.random.RandomState(7), prefetch=0, **cam)
        for step in range(3):
            a, b = next(ds), next(hand)
            assert torch.equal(a["pixels"], b["pixels"]) and tuple(a["pixels"].shape) == (16, 3)
            for f in ("origins", "directions", "viewdirs"):
                assert torch.equal(getattr(a["rays"], f), getattr(b["rays"], f)), (dataset, step, f)
                assert torch.equal(getattr(a["env_rays"], f), getattr(b["env_rays"], f)) and tuple(getattr(a["env_rays"], f).shape) == (4, 4, 3)
        assert ds.batcher.train_it == 3 and ds.batcher.out_of_range_indices() == 0


def test_masks(tmp_path):
    """load_masks at factor 2 is [::2, ::2] of the written masks (at factor 0 the masks themselves), in frame order, and one of them goes
    through evaluate.apply_mask with its view."""
    from samplenerfro_amd import datasets, evaluate
    wrote = SF.write_blender(str(tmp_path))
    masks = SF.write_masks(str(tmp_path), "blender")
    flags = flags_of("blender", str(tmp_path), factor=2)
    m = datasets.load_masks(str(tmp_path), "test", flags, device=DEV)
    assert m.dtype == torch.uint8 and m.is_cuda and same(m, np.ascontiguousarray(masks["test"][:, ::2, ::2]))
    assert same(datasets.load_masks(str(tmp_path), "train", flags_of("blender", str(tmp_path), skip_frames=2), device=DEV), masks["train"][::2])
    ds = datasets.get_dataset("test", flags, device=DEV)
    b = next(ds)
    pred = torch.full_like(b["pixels"], 0.5)
    p, q = evaluate.apply_mask(pred, b["pixels"], m[0], "mask")
    on = (masks["test"][0, ::2, ::2] > 0).astype(F32)[..., None]
    assert same(q, SF.prepare_reference(wrote["test"], 2)[0] * on) and same(p, np.full((SF.H // 2, SF.W // 2, 3), 0.5, F32) * on)
    SF.write_opencv(str(tmp_path / "cv"))
    cv_masks = SF.write_masks(str(tmp_path / "cv"), "opencv")
    assert same(datasets.load_masks(str(tmp_path / "cv"), "test", flags_of("opencv", str(tmp_path / "cv")), device=DEV), cv_masks["test"])
