"""SSIM and the evaluation loop's files, without a GPU.

- tests/helpers/ssim_ref.py (the float64 restatement every device test is held to) against tests/golden/ssim_reference.npz, which
  tests/golden/make_ssim_reference.py computed by running the reference's own compute_ssim text (re-run here where the reference exists);
- known answers of the restatement (identical, constant and affine images);
- rnerf_ssim's argument checks and compute_ssim's shape checks, which need no device;
- utils.save_img and evaluate.write_metric_files against the formats of rnerf/utils.py:474-488 and eval.py:207-215, byte for byte."""
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_ssim_reference as M      # noqa: E402
import ssim_ref                      # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "ssim_reference.npz")


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(FIXTURE) < 100 * 1024
    d = np.load(FIXTURE)
    assert d["out_default"].shape == (2,) and d["out_default_map"].shape == (2, 14, 21, 3)
    assert sorted(k[4:] for k in d.files if k.startswith("out_")) == sorted(M.CASES)


@pytest.mark.parametrize("case", sorted(M.CASES))
def test_float64_restatement_equals_the_references_vectors(case):
    d = np.load(FIXTURE)
    src, kw = M.CASES[case]
    a, b = d[f"in_{src}_0"], d[f"in_{src}_1"]
    got = ssim_ref.ssim(a, b, **kw)
    want = d[f"out_{case}"]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.max(np.abs(got[ok] - want[ok]), initial=0.0) <= 1e-12


def test_fixture_inputs_take_every_branch():
    d = np.load(FIXTURE)
    # the negative-slope affine pair reaches sign(sigma01) = -1 with |sigma01| clipped to sqrt(sigma00 sigma11)
    assert np.all(d["out_affine_negative"] < 0)
    # one NaN pixel at (7, 9) of channel 1 with a 5-wide window: NaN exactly on the windows covering it, in that channel
    nan = np.isnan(d["out_nan"])
    want = np.zeros_like(nan)
    want[3:8, 5:10, 1] = True
    assert np.array_equal(nan, want)


def test_generator_reproduces_the_committed_file():
    if M.source_sha256() is None:
        pytest.skip("the reference checkout is not on this machine")
    assert M.check(FIXTURE)


def test_known_answer_identical_images():
    x = np.random.default_rng(1).uniform(0, 1, (2, 20, 23, 3))
    np.testing.assert_allclose(ssim_ref.ssim(x, x, 1.0, return_map=True), 1.0, rtol=0, atol=1e-13)
    np.testing.assert_allclose(ssim_ref.ssim(x, x, 1.0), 1.0, rtol=0, atol=1e-13)


def test_known_answer_constant_images():
    a, b, c1 = 0.3, 0.8, (0.01 * 1.0) ** 2
    got = ssim_ref.ssim(np.full((15, 17, 2), a), np.full((15, 17, 2), b), 1.0, return_map=True)
    np.testing.assert_allclose(got, (2 * a * b + c1) / (a * a + b * b + c1), rtol=1e-12, atol=0)


@pytest.mark.parametrize("slope", [0.6, -0.7])
def test_known_answer_affine_pair_gives_the_contrast_structure_term(slope):
    rng = np.random.default_rng(2)
    x = rng.uniform(0, 1, (19, 21, 3))
    y = slope * x + 0.2
    fs, c1, c2 = 7, 1e-4, 9e-4
    got = ssim_ref.ssim(x, y, 1.0, filter_size=fs, return_map=True)
    filt = ssim_ref.gaussian_filter(fs, 1.5)
    mu0, mu1 = ssim_ref.blur(x, filt), ssim_ref.blur(y, filt)
    var = ssim_ref.blur(x * x, filt) - mu0 * mu0
    lum = (2 * mu0 * mu1 + c1) / (mu0 * mu0 + mu1 * mu1 + c1)
    cs = (2 * slope * var + c2) / ((1 + slope * slope) * var + c2)
    np.testing.assert_allclose(got / lum, cs, rtol=1e-9, atol=0)


def test_argument_errors_do_not_need_a_gpu(lib_path):
    import ctypes
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)

    def call(n, H, W, C, fs, sigma=1.5):
        return lib.rnerf_ssim(p, p, n, H, W, C, fs, sigma, 1.0, 0.01, 0.03, None, p, p, None)

    for fs in (0, 32):
        assert call(1, 40, 40, 3, fs) == -1 and b"filter_size" in lib.rnerf_last_error()
        assert lib.rnerf_ssim_workspace_bytes(1, 40, 40, 3, fs) == 0
    assert call(1, 10, 40, 3, 11) == -1 and b"smaller than the window" in lib.rnerf_last_error()
    assert call(1, 40, 10, 3, 11) == -1 and b"smaller than the window" in lib.rnerf_last_error()
    assert lib.rnerf_ssim_workspace_bytes(1, 10, 40, 3, 11) == 0
    assert call(1, 40, 40, 3, 11, sigma=0.0) == -1 and b"filter_sigma" in lib.rnerf_last_error()
    assert lib.rnerf_ssim(None, p, 1, 40, 40, 3, 11, 1.5, 1.0, 0.01, 0.03, None, p, p, None) == -1
    assert lib.rnerf_ssim(p, p, 1, 40, 40, 3, 11, 1.5, 1.0, 0.01, 0.03, None, None, p, None) == -1     # neither map nor mean
    assert lib.rnerf_ssim(p, p, 1, 40, 40, 3, 11, 1.5, 1.0, 0.01, 0.03, None, p, None, None) == -1     # a mean without a workspace
    # one fp64 partial per 16 x 64-float tile at the default window: 800 x 800 x 3 (a 790 x 2370-float map) -> 50 x 38 tiles
    assert lib.rnerf_ssim_workspace_bytes(1, 800, 800, 3, 11) == 8 * 50 * 38
    assert lib.rnerf_ssim_workspace_bytes(4, 800, 800, 3, 11) == 4 * 8 * 50 * 38
    assert lib.rnerf_ssim_workspace_bytes(1, 31, 31, 3, 31) > 0


def test_compute_ssim_rejects_bad_shapes_before_any_device_work():
    from samplenerfro_amd import utils
    a = np.zeros((20, 20, 3), np.float32)
    with pytest.raises(ValueError):
        utils.compute_ssim(a, np.zeros((20, 21, 3), np.float32), max_val=1.0)
    with pytest.raises(ValueError):
        utils.compute_ssim(a[0], a[0], max_val=1.0)
    with pytest.raises(ValueError):
        utils.compute_ssim(a, a, max_val=1.0, filter_size=21)
    with pytest.raises(ValueError):
        utils.compute_ssim(a, a, max_val=1.0, filter_size=0)


def _png_bytes_of(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "PNG")
    return buf.getvalue()


def test_save_img_matches_the_reference_format(tmp_path):
    from PIL import Image
    from samplenerfro_amd import utils
    rng = np.random.default_rng(3)
    rgb = rng.uniform(-0.2, 1.2, (9, 11, 3)).astype(np.float32)
    rgb[0, 0] = [0.999, 1.0, 0.5]
    disp = rng.uniform(0, 1, (9, 11)).astype(np.float32)
    for name, img in (("rgb.png", rgb), ("disp.png", disp)):
        utils.save_img(img, str(tmp_path / name))
        want = (np.clip(img, 0., 1.) * 255.).astype(np.uint8)          # rnerf/utils.py:484-485: clip, scale, truncate
        assert (tmp_path / name).read_bytes() == _png_bytes_of(want)
        assert np.array_equal(np.asarray(Image.open(tmp_path / name)), want)
    assert tuple(np.asarray(Image.open(tmp_path / "rgb.png"))[0, 0]) == (254, 255, 127)
    img8 = rng.integers(0, 256, (5, 6, 3), dtype=np.uint8)
    utils.save_img(img8, str(tmp_path / "raw.png"), to8b=False)
    assert (tmp_path / "raw.png").read_bytes() == _png_bytes_of(img8)


def test_metric_files_match_eval_py_byte_for_byte(tmp_path):
    from samplenerfro_amd import evaluate
    psnrs = [23.4567890123, 19.0, 31.25]
    ssims = [0.8123456789, 0.5, 0.9999]
    evaluate.write_metric_files(str(tmp_path), 250000, psnrs, ssims)
    assert (tmp_path / "psnrs_250000.txt").read_text() == "23.4567890123 19.0 31.25"
    assert (tmp_path / "ssims_250000.txt").read_text() == "0.8123456789 0.5 0.9999"
    assert (tmp_path / "psnr.txt").read_text() == "{}".format(np.mean(np.array(psnrs)))
    assert (tmp_path / "ssim.txt").read_text() == "{}".format(np.mean(np.array(ssims)))
    assert sorted(os.listdir(tmp_path)) == ["psnr.txt", "psnrs_250000.txt", "ssim.txt", "ssims_250000.txt"]
