"""Host side of the scene loaders (no GPU): the argument checks of rnerf_images_prepare, the stated factor-2 deviation from the
reference's float chain, the consistency of the example fixtures, and samplenerfro_amd.datasets' loaders up to the device call — which
JSON, which frames, which files, the cameras — against what the reference's own loaders computed on the same tiny scenes
(tests/golden/scene_loader_reference.npz, made by tests/golden/make_scene_loader_reference.py from tests/helpers/scene_fixture.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import scene_fixture as SF      # noqa: E402

from samplenerfro_amd import _lib, datasets, utils      # noqa: E402

F32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "scene_loader_reference.npz"))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    import make_scene_loader_reference as M
    return M.write_scenes(str(tmp_path_factory.mktemp("scenes")))


def flags_of(dataset, data_dir, **over):
    return utils.default_flags(**dict(dict(dataset=dataset, data_dir=data_dir, factor=0, white_bkgd=False), **over))


def test_images_prepare_argument_errors_do_not_need_a_gpu(lib_path):
    lib = _lib.load()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    err = lambda: lib.rnerf_last_error()
    call = lambda src=p, n=2, H=8, W=12, C=4, factor=1, white=0, dst=q: lib.rnerf_images_prepare(src, n, H, W, C, factor, white, dst, None)
    assert call(src=None) == -1 and b"rnerf_images_prepare" in err() and b"null pointer" in err()
    assert call(dst=None) == -1 and b"rnerf_images_prepare" in err() and b"null pointer" in err()
    for C in (0, 1, 2, 5):
        assert call(C=C) == -1 and b"rnerf_images_prepare: C must be" in err()
    for factor in (0, 3, 4, -1):
        assert call(factor=factor) == -1 and b"rnerf_images_prepare: factor" in err()
    assert call(H=7, factor=2) == -1 and b"rnerf_images_prepare" in err() and b"even" in err()
    assert call(W=11, factor=2) == -1 and b"rnerf_images_prepare" in err() and b"even" in err()
    assert call(C=3, white=1) == -1 and b"rnerf_images_prepare: white_bkgd needs" in err()
    assert call(white=2) == -1 and b"rnerf_images_prepare" in err()
    for kw in (dict(n=0), dict(H=0), dict(W=0), dict(n=-1)):
        assert call(**kw) == -1 and b"rnerf_images_prepare" in err()
    assert call(n=1 << 40) == -1 and b"2^39" in err()
    assert call(src=ctypes.c_void_p(4098)) == -1 and b"aligned" in err()            # RGBA pixels are read as 32-bit words


def _emulate_factor2(q):
    """The definition (include/rnerf.h) on quadruples uint8 [N, 4]: float32(exact integer sum) / 1020."""
    return q.astype(np.uint32).sum(axis=1).astype(F32) / F32(1020.0)


def test_the_factor_2_mean_is_within_the_derived_bound_of_the_references_float_chain():
    """The reference at factor 2 divides every 8-bit value by 255 in float32 and lets cv2.INTER_AREA average the four floats; the product
    divides the exact integer sum by 1020.  cv2's association order is not pinned (cv2 is not installed where this was written), so the
    chain is tried in the three orders four values can be paired in, and sequentially.  Derived bound: four conversions off by at most 2^-25
    each, three additions by at most 2^-23 each (sums below 4), times 1/4, plus the product's own rounding of 2^-25: below 2^-22.
    Observed maximum on these 10^6 seeded quadruples and the two corners: 2^-24 (5.96046448e-08) in each of the three pairwise orders,
    2^-23 (1.1920929e-07) in the sequential one."""
    rng = np.random.default_rng(20261019)
    q = np.concatenate([rng.integers(0, 256, (1_000_000, 4), dtype=np.uint8), np.zeros((1, 4), np.uint8), np.full((1, 4), 255, np.uint8)])
    ours = _emulate_factor2(q)
    f = q.astype(F32) / F32(255.0)
    a, b, c, d = f[:, 0], f[:, 1], f[:, 2], f[:, 3]
    quarter = F32(0.25)
    chains = {"(a+b)+(c+d)": ((a + b) + (c + d)) * quarter, "(a+c)+(b+d)": ((a + c) + (b + d)) * quarter, "(a+d)+(b+c)": ((a + d) + (b + c)) * quarter,
              "((a+b)+c)+d": (((a + b) + c) + d) * quarter}
    worst = 0.0
    for name, chain in chains.items():
        assert chain.dtype == F32
        delta = float(np.abs(ours.astype(np.float64) - chain.astype(np.float64)).max())
        print(f"factor 2 vs the float chain {name}: max |delta| = {delta:.9g} = 2^{np.log2(delta):.3f}")
        assert delta <= 2.0 ** -22, (name, delta)
        worst = max(worst, delta)
    assert worst > 0.0                                   # the two are not the same function: the deviation is real and stated
    assert ours[-2] == 0.0 and ours[-1] == 1.0 and all(ch[-2] == 0.0 and ch[-1] == 1.0 for ch in chains.values())


def test_the_example_window_is_a_block_of_the_example_image_fixture():
    """The definition applied to example_scene.npz's 64 x 96 window equals rgba_sum4 / 1020 of the matching 32 x 48 block of
    example_image.npz bit for bit.  (The view is rendered against a sky dome: its alpha is 255 everywhere, so the white composite returns
    the colours; partial alpha is the synthetic scenes' part.)"""
    ex = np.load(os.path.join(GOLDEN, "example_scene.npz"))
    win, (r, c) = ex["window"], (int(v) for v in ex["origin"])
    assert win.shape == (64, 96, 4) and win.dtype == np.uint8 and r % 2 == 0 and c % 2 == 0
    assert len(np.unique(win[..., :3])) > 100                                    # not a flat patch of background
    s4 = np.load(os.path.join(GOLDEN, "example_image.npz"))["rgba_sum4"][r // 2:r // 2 + 32, c // 2:c // 2 + 48]
    mine = win.astype(np.uint32).reshape(32, 2, 48, 2, 4).sum(axis=(1, 3))
    assert np.array_equal(mine, s4)
    want = s4.astype(F32) / F32(1020.0)
    assert np.array_equal(SF.prepare_reference(win[None], factor=2)[0], want[..., :3])
    x = want
    assert np.array_equal(SF.prepare_reference(win[None], factor=2, white_bkgd=True)[0], x[..., :3] * x[..., 3:] + (F32(1.0) - x[..., 3:]))
    assert ex["transform_matrix"].shape == (4, 4) and 0.0 < float(ex["camera_angle_x"]) < np.pi


CASE_FLAGS = {
    "blender_test": ("blender", "blender", "test", {}), "blender_train_skip2": ("blender", "blender", "train", dict(skip_frames=2)),
    "blender_test_eval_train": ("blender", "blender", "test", dict(eval_train=True)),
    "opencv_test": ("opencv", "opencv", "test", {}), "opencv_train_skip2": ("opencv", "opencv", "train", dict(skip_frames=2)),
    "opencv_test_eval_train": ("opencv", "opencv", "test", dict(eval_train=True)), "opencv_rgb_test": ("opencv_rgb", "opencv", "test", {}),
    "nsvf_test": ("nsvf", "nsvf", "test", {}), "nsvf_train": ("nsvf", "nsvf", "train", {}),
}


@pytest.mark.parametrize("case", sorted(CASE_FLAGS))
def test_the_index_is_the_references(case, ref, scenes):
    """Frames, cameras and decoded pixels of every case, against the reference's loader: camtoworlds, focal and cam_mat exactly; the
    decoded uint8 / 255 in float32 equals the reference's images (white_bkgd off: the first three channels)."""
    scene, dataset, split, over = CASE_FLAGS[case]
    idx = datasets.INDEXERS[dataset](split, flags_of(dataset, scenes[scene], **over))
    n, h, w = int(ref[f"{case}_n_examples"]), int(ref[f"{case}_h"]), int(ref[f"{case}_w"])
    assert len(idx.files) == n and idx.factor == 1 and idx.white_bkgd is False
    assert idx.camtoworlds.dtype == F32 and np.array_equal(idx.camtoworlds, ref[f"{case}_camtoworlds"])
    cam = idx.camera(w)
    if dataset == "opencv":
        assert np.array_equal(np.array(cam["cam_mat"], np.float64), ref[f"{case}_cam_mat"]) and "focal" not in cam
    else:
        assert float(cam["focal"]) == float(ref[f"{case}_focal"]) and "cam_mat" not in cam
    u8 = datasets.decode_views(idx.files)
    assert u8.dtype == np.uint8 and u8.shape[:3] == (n, h, w) and u8.shape[3] == (3 if scene == "opencv_rgb" else 4)
    assert np.array_equal(SF.prepare_reference(u8), ref[f"{case}_images"])


def test_the_written_pixels_come_back(tmp_path):
    wrote = SF.write_blender(str(tmp_path))
    for split in ("train", "test"):
        idx = datasets.blender_index(split, flags_of("blender", str(tmp_path)))
        assert [os.path.basename(f) for f in idx.files] == [f"r_{i}.png" for i in range(SF.SPLITS[split])]
        assert np.array_equal(datasets.decode_views(idx.files), wrote[split])
    a = wrote["train"][..., 3]
    assert a.min() == 0 and a.max() == 255 and ((a > 0) & (a < 255)).any()


def test_factor_and_focal(scenes):
    b2 = datasets.blender_index("test", flags_of("blender", scenes["blender"], factor=2))
    assert b2.factor == 2
    assert b2.camera(SF.W // 2)["focal"] == .5 * (SF.W // 2) / np.tan(.5 * SF.CAMERA_ANGLE_X)          # the halved width
    n2 = datasets.nsvf_index("test", flags_of("nsvf", scenes["nsvf"], factor=2))
    assert n2.factor == 2 and n2.camera(SF.W // 2)["focal"] == SF.NSVF_INTRINSICS[0] * 0.5
    for neg in (0, -1):                                                                                # as in the reference: nothing resized
        assert datasets.blender_index("test", flags_of("blender", scenes["blender"], factor=neg)).factor == 1


def test_loader_errors(scenes, tmp_path):
    with pytest.raises(ValueError, match="Blender dataset only supports factor=0 or 2, 4 set."):
        datasets.blender_index("test", utils.default_flags(data_dir=scenes["blender"]))               # the default factor, as in the reference
    with pytest.raises(ValueError, match="only supports factor=0 or 2, 3 set."):
        datasets.nsvf_index("test", flags_of("nsvf", scenes["nsvf"], factor=3))
    for factor in (1, 2, 4):
        with pytest.raises(ValueError, match=f"Opencv dataset does not support factor, {factor} set."):
            datasets.opencv_index("test", flags_of("opencv", scenes["opencv"], factor=factor))
    for dataset in ("blender", "opencv", "nsvf"):
        with pytest.raises(ValueError, match="render_path cannot be used"):
            datasets.INDEXERS[dataset]("test", flags_of(dataset, scenes[dataset], render_path=True))
        with pytest.raises(ValueError, match="split argument"):
            datasets.INDEXERS[dataset]("holdout", flags_of(dataset, scenes[dataset]))
    with pytest.raises(NotImplementedError, match="no shipped config uses it.*NDC rays"):
        datasets.get_dataset("train", flags_of("llff", scenes["blender"]))
    with pytest.raises(KeyError):
        datasets.get_dataset("train", flags_of("dtu", scenes["blender"]))
    with pytest.raises(FileNotFoundError):
        datasets.blender_index("val", flags_of("blender", scenes["blender"]))                          # the scenes have no transforms_val.json
    # mixed sizes and mixed channel counts within a scene
    SF.write_blender(str(tmp_path / "a"))
    SF.write_blender(str(tmp_path / "b"), size=(8, 14))
    SF.write_blender(str(tmp_path / "c"), channels=3)
    fa, fb, fc = (datasets.blender_index("train", flags_of("blender", str(tmp_path / k))).files for k in "abc")
    with pytest.raises(ValueError, match="one size and channel count"):
        datasets.decode_views([fa[0], fb[1]])
    with pytest.raises(ValueError, match="one size and channel count"):
        datasets.decode_views([fa[0], fc[1]])
    from PIL import Image
    Image.fromarray(np.zeros((8, 12), np.uint8)).save(str(tmp_path / "grey.png"))
    with pytest.raises(ValueError, match="8-bit RGB or RGBA"):
        datasets.decode_views([str(tmp_path / "grey.png")])


def test_default_flags_carry_the_scene_flags():
    f = utils.default_flags()
    assert (f.dataset, f.data_dir, f.factor, f.skip_frames, f.eval_train, f.render_path, f.use_pixel_centers, f.precrop_iters, f.precrop_frac,
            f.batching) == ("blender", None, 4, 1, False, False, False, 0, 0.5, "single_image")


def test_the_decode_pool_is_not_sized_from_the_machine():
    src = open(os.path.join(ROOT, "samplenerfro_amd", "datasets.py")).read()
    assert datasets.DECODE_WORKERS <= 8 and "cpu_count" not in src


def test_the_committed_fixture_is_what_the_reference_computes_today():
    """Where the reference is present, the fixture script is run again and must reproduce the committed file (elsewhere there is nothing
    to compare with: the committed file is the record)."""
    import make_scene_loader_reference as M
    if M.base.source_sha256() is None:
        return
    assert M.check()
