"""LDR-FLIP without a GPU.

- tests/helpers/flip_ref.py (the float64 restatement the device tests use for sizes the fixture cannot hold) against
  tests/golden/flip_reference.npz, which tests/golden/make_flip_reference.py computed by running the reference's own compute_ldrflip
  text (re-run here where the reference exists);
- rnerf_flip's argument checks, its workspace query and compute_flip's shape checks, which need no device;
- evaluate.write_metric_files with FLIP values.

Tolerances come from the fixture: floor_<case> / floor_mean_<case> are the max / mean distance between two evaluations of the reference's
text that differ only in the filter's accumulation precision (float64 / float32).  Class A (the images differ everywhere): max error
<= 4 floor + 1e-6 and mean error <= 2 floor_mean + 1e-6, the margins of tests/test_gpu_ssim.py.  Class B (partly identical images): the
metric's last step deltaE_c ^ (1 - deltaE_f) is ill-conditioned where the colour difference is tiny but not zero, so no per-pixel bar is
a property of a correct implementation; the mean rule, the exact zeros and the NaN mask are."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_flip_reference as M      # noqa: E402
import flip_ref                      # noqa: E402
from flip_checks import FIXTURE, check_against_fixture, load_case      # noqa: E402


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(FIXTURE) < 150 * 1024
    d = np.load(FIXTURE)
    assert sorted(k[4:] for k in d.files if k.startswith("out_")) == sorted(M.keys())
    assert d["out_noise_lo"].shape == (48, 64) and d["out_batch_hi"].shape == (2, 24, 32)
    assert flip_ref.radii(M.PPD["hi"]) == (10, 9) and flip_ref.radii(M.PPD["lo"]) == (1, 1)
    assert M.PPD["hi"] == flip_ref.PPD_DEFAULT and M.PPD["lo"] == flip_ref.PPD_SUMMARY
    for k in M.keys():
        assert 0 < float(d[f"floor_mean_{k}"]) <= float(d[f"floor_{k}"]) < 1e-2


@pytest.mark.parametrize("key", M.keys())
def test_float64_restatement_against_the_references_vectors(key):
    a, b, ppd, *_ = load_case(key)
    with np.errstate(invalid="ignore"):
        check_against_fixture(key, flip_ref.flip(a, b, ppd))


def test_fixture_inputs_take_every_branch():
    d = np.load(FIXTURE)
    for p, r in (("lo", 1), ("hi", 10)):
        # one NaN pixel: NaN exactly on the square of the spatial radius around it
        nan = np.isnan(d[f"out_nan_{p}"])
        want = np.zeros_like(nan)
        y, x, _ = M.NAN_AT
        want[y - r:y + r + 1, x - r:x + r + 1] = True
        assert np.array_equal(nan, want)
        # the half-identical pair: zero on the left beyond the footprint, errors on the right; both redistribution branches are taken
        half = d[f"out_half_identical_{p}"]
        assert np.all(half[:, :32 - r] == 0) and np.all(half[:, 32:] > 0)
    assert d["out_noise_lo"].max() > 0.99 and d["out_smooth_noised_hi"].min() < 0.05


def test_generator_reproduces_the_committed_file():
    if M.source_sha256() is None:
        pytest.skip("the reference checkout is not on this machine")
    assert M.check(FIXTURE)


def test_restatement_known_answers():
    x = np.random.default_rng(1).uniform(0, 1, (2, 20, 23, 3)).astype(np.float32)
    for dt in (np.float64, np.float32):
        assert np.all(flip_ref.flip(x, x, M.PPD["lo"], dtype=dt) == 0)
    # black against white at a coarse sampling: HyAB 100 of cmax^(1/0.7) = 203.4 -> the upper redistribution branch, no features in a
    # constant image, so the error is deltaE_c itself
    m = flip_ref.flip(np.zeros((8, 9, 3)), np.ones((8, 9, 3)), M.PPD["lo"])
    cm = flip_ref.cmax()
    want = 0.95 + (100 ** 0.7 - 0.4 * cm) / (0.6 * cm) * 0.05
    np.testing.assert_allclose(m, want, rtol=1e-5)
    assert abs(cm ** (1 / 0.7) - 203.4) < 0.2
    for f in flip_ref.spatial_filters(M.PPD["hi"]):
        assert f.shape == (21, 21) and abs(f.sum() - 1) < 1e-12
    for f in flip_ref.feature_filters(M.PPD["hi"]):
        assert f.shape == (19, 19) and abs(f[f > 0].sum() - 1) < 1e-12 and abs(f[f < 0].sum() + 1) < 1e-12


def test_argument_errors_and_workspace_do_not_need_a_gpu(lib_path):
    import ctypes
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    hi, lo = M.PPD["hi"], M.PPD["lo"]

    assert lib.rnerf_flip(None, p, 1, 40, 40, hi, p, p, p, None) == -1 and b"null pointer" in lib.rnerf_last_error()
    assert lib.rnerf_flip(p, None, 1, 40, 40, hi, p, p, p, None) == -1
    assert lib.rnerf_flip(p, p, 1, 40, 40, hi, None, None, p, None) == -1                # neither map nor mean
    assert lib.rnerf_flip(p, p, 1, 40, 40, hi, None, p, None, None) == -1 and b"workspace" in lib.rnerf_last_error()
    assert lib.rnerf_flip(p, p, 1, 40, 40, hi, None, p, ctypes.c_void_p(260), None) == -1 and b"8-byte" in lib.rnerf_last_error()
    for n, H, W in ((0, 40, 40), (1, 0, 40), (1, 40, 0)):
        assert lib.rnerf_flip(p, p, n, H, W, hi, p, p, p, None) == -1
        assert lib.rnerf_flip_workspace_bytes(n, H, W, hi) == 0
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        assert lib.rnerf_flip(p, p, 1, 40, 40, bad, p, p, p, None) == -1 and b"pixels_per_degree" in lib.rnerf_last_error()
        assert lib.rnerf_flip_workspace_bytes(1, 40, 40, bad) == 0
    # the header's formula: one fp64 partial per 16 x 64 tile, then 14 planes; the same at every supported pixels_per_degree
    for ppd in (hi, lo):
        assert lib.rnerf_flip_workspace_bytes(1, 800, 800, ppd) == 8 * 50 * 13 + 56 * 800 * 800
        assert lib.rnerf_flip_workspace_bytes(3, 37, 53, ppd) == 3 * (8 * 3 * 1 + 56 * 37 * 53)
    # the spatial radius ceil(3 sqrt(0.04 / (2 pi^2)) ppd) is capped at 15: 15 up to ppd 111.07, 16 above
    edge = 15 / (3 * np.sqrt(0.04 / (2 * np.pi ** 2)))
    assert flip_ref.radii(edge - 1e-6)[0] == 15 and flip_ref.radii(edge + 1e-6)[0] == 16
    assert lib.rnerf_flip_workspace_bytes(1, 800, 800, edge - 1e-6) > 0
    assert lib.rnerf_flip_workspace_bytes(1, 800, 800, edge + 1e-6) == 0
    assert lib.rnerf_flip(p, p, 1, 800, 800, edge + 1e-6, p, p, p, None) == -3           # RNERF_ERR_UNSUPPORTED
    assert b"radii 16 and %d" % flip_ref.radii(edge + 1e-6)[1] in lib.rnerf_last_error()
    # the radii the library derives for the two values the reference uses are not an error and not at the cap; a pixels_per_degree whose
    # detectors vanish is unsupported too
    assert lib.rnerf_flip_workspace_bytes(1, 40, 40, 0.01) == 0 and lib.rnerf_flip(p, p, 1, 40, 40, 0.01, p, p, p, None) == -3


def test_compute_flip_rejects_bad_shapes_before_any_device_work():
    from samplenerfro_amd import utils
    a = np.zeros((20, 20, 3), np.float32)
    with pytest.raises(ValueError):
        utils.compute_flip(a, np.zeros((20, 21, 3), np.float32))
    with pytest.raises(ValueError):
        utils.compute_flip(a[..., :2], a[..., :2])
    with pytest.raises(ValueError):
        utils.compute_flip(a[0], a[0])
    with pytest.raises(ValueError):
        utils.compute_flip(a, a, pixels_per_degree=0.0)
    assert utils.FLIP_PPD_SUMMARY == flip_ref.PPD_SUMMARY and utils.FLIP_PPD_DEFAULT == flip_ref.PPD_DEFAULT


def test_metric_files_with_flip_values(tmp_path):
    from samplenerfro_amd import evaluate
    psnrs, ssims, flips = [23.4567890123, 19.0], [0.8123456789, 0.5], [0.123456789, 0.25]
    evaluate.write_metric_files(str(tmp_path), 7, psnrs, ssims, flips)
    assert (tmp_path / "flips_7.txt").read_text() == "0.123456789 0.25"
    assert (tmp_path / "flip.txt").read_text() == "{}".format(np.mean(np.array(flips)))
    assert (tmp_path / "ssims_7.txt").read_text() == "0.8123456789 0.5"
    assert sorted(os.listdir(tmp_path)) == ["flip.txt", "flips_7.txt", "psnr.txt", "psnrs_7.txt", "ssim.txt", "ssims_7.txt"]
