"""samplenerfro_amd.errmap on the device against tests/helpers/errmap_ref.py (float64 maps, exact bytes) and against what the reference's
own text recorded in tests/golden/errmap_reference.npz, at the fixture's three shapes: 11 x 11 (one window), 29 x 33 (the channel triple
at flat output columns 63-65 straddles the 64-column SSIM tile, 19 output rows span two row tiles) and 45 x 70 (values outside [0, 1]).

Tolerances.  Maps: max(4 e_ref, 1e-6) absolute, e_ref the largest error of the reference's own float32 run against float64 on the same
input (measured by tests/golden/make_errmap_reference.py, stored in the fixture): a different float32 summation order over the 121 taps
and nothing more should separate the device from the reference.  The SSIM value is a mean of its map, so the map's bound holds for it.
The PSNR value is -10 log10(mse): the device's mse is a float64 sum of float32 squares rounded once (each square carries the rounding of
the difference, twice, and its own: 3 x 2^-24 relative, plus 2^-24 for the final rounding), so 10 / ln 10 x 4 x 2^-24 = 1.04e-6, plus
float32 sqrt, log10 and the product at 8 ulp of the value together.  Bytes are exact.

Measured on an MI355X (the tests print every figure): SSIM map 1.3e-7 / 7.3e-7 / 1.8e-6 from float64 at the three shapes (bounds 3.4e-6 /
2.1e-5 / 2.1e-5), squared-error map 1.5e-9 - 2.0e-8 (bound 1e-6), PSNR value 0.9e-6 - 1.3e-6 dB (bound 1.7e-5 - 2.2e-5); no colour index
differs from the reference's recorded bytes.  Timing: tools/errmap_time.py, DESIGN.md 3.14."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import errmap_ref as R               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("11x11", "29x33", "45x70")
MAPS = ("psnr", "ssim", "flip")
EPS32 = 2.0 ** -24


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(ROOT, "tests", "golden", "errmap_reference.npz"))


@pytest.fixture(scope="module")
def device_maps(fix):
    """case -> (reference, test, error_maps read back), computed once."""
    from samplenerfro_amd import errmap
    out = {}
    for case in CASES:
        ref, test = fix[f"in_{case}_ref"], fix[f"in_{case}_test"]
        out[case] = (ref, test, {k: v.cpu().numpy() for k, v in errmap.error_maps(ref, T(test)).items()})
    return out


def indices(colour_bytes):
    """The colour index of every pixel of a coloured map (the table's rows are distinct)."""
    lut = R.magma_lut().astype(np.int64)
    key = lambda c: (c[..., 0] * 256 + c[..., 1]) * 256 + c[..., 2]
    order = np.argsort(key(lut))
    pos = np.searchsorted(key(lut)[order], key(colour_bytes.astype(np.int64)))
    idx = order[pos]
    assert np.array_equal(lut[idx], colour_bytes)
    return idx


@pytest.mark.parametrize("case", CASES)
def test_maps_and_values_against_float64(fix, device_maps, case):
    from samplenerfro_amd import utils as U
    ref, test, got = device_maps[case]
    H, W = ref.shape[:2]
    mse_map, mse = R.mse_map(ref, test)
    ssim_map, ssim = R.ssim_summary(ref, test)
    assert got["psnr"].shape == (H, W) and got["ssim"].shape == (H - 10, W - 10) and got["flip"].shape == (H, W)
    assert all(got[k].dtype == np.float32 for k in got) and all(got[f"{k}_value"].shape == () for k in MAPS)
    for name, want in (("psnr", mse_map), ("ssim", ssim_map)):
        bound = max(4 * float(fix[f"e_ref_{name}_{case}"]), 1e-6)
        err = float(np.max(np.abs(got[name] - want)))
        print(f"{case} {name}: max error {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (name, err, bound)
    err, bound = abs(float(got["ssim_value"]) - ssim), max(4 * float(fix[f"e_ref_ssim_{case}"]), 1e-6)
    print(f"{case} ssim value: error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    want = R.psnr_value(mse)
    err, bound = abs(float(got["psnr_value"]) - want), 10 / math.log(10) * 4 * EPS32 + 8 * 2 * EPS32 * max(abs(want), 1.0)
    print(f"{case} psnr value {want:.6f}: error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    flip_map = U.compute_flip(T(ref), T(test), U.FLIP_PPD_SUMMARY, return_map=True).cpu().numpy()
    assert np.array_equal(got["flip"], flip_map)
    assert float(got["flip_value"]) == float(U.compute_flip(T(ref), T(test), U.FLIP_PPD_SUMMARY).cpu())


@pytest.mark.parametrize("case", CASES)
def test_sheet_and_colorize_bytes_are_exact(device_maps, case):
    from samplenerfro_amd import errmap
    ref, test, got = device_maps[case]
    H, W = ref.shape[:2]
    for names in (("ssim",), MAPS):                                   # K = 1 (a map smaller than the image) and K = 3
        maps = [got[n] for n in names]
        sheet = errmap.sheet(T(ref), test, [T(m) for m in maps])
        assert sheet.dtype == torch.uint8 and sheet.is_cuda and tuple(sheet.shape) == (H, (2 + len(maps)) * (W + 5), 3)
        assert np.array_equal(sheet.cpu().numpy(), R.sheet(ref, test, maps)), names
    for n in MAPS:
        col = errmap.colorize(T(got[n]))
        assert col.dtype == torch.uint8 and np.array_equal(col.cpu().numpy(), R.colorize(got[n])), n
    three = errmap.sheet(ref, test, [got[n] for n in MAPS]).cpu().numpy()
    for n, panel in zip(MAPS, errmap.panels(three, [got[n].shape for n in MAPS])):
        assert np.array_equal(panel, R.colorize(got[n])), n           # the errmap PNGs are slices of the sheet


def test_nan_and_out_of_range_bytes(device_maps):
    from samplenerfro_amd import errmap
    ref, test, got = device_maps["29x33"]
    ref, test = ref.copy(), test.copy()
    ref[3, 4, 1], ref[0, 0, 0], test[5, 6, 0], test[7, 8, 2], test[28, 32, 2], ref[9, 9, 0] = np.nan, -0.0, -0.5, 3.0, np.inf, -np.inf
    maps = [got["psnr"].copy(), got["ssim"].copy(), got["flip"].copy(), got["ssim"][:5, :7].copy()]
    maps[0][0, 0], maps[0][1, 1], maps[0][2, 2], maps[0][28, 32] = np.nan, -1.0, 7.0, np.inf
    maps[1][18, 22], maps[1][0, 5], maps[3][4, 6] = -np.inf, np.nan, 1.0
    maps[2][:, 0] = np.linspace(-0.1, 1.1, 29, dtype=np.float32)
    want = R.sheet(ref, test, maps)
    assert np.array_equal(errmap.sheet(ref, test, maps).cpu().numpy(), want)
    assert want[3, 4].tolist()[1] == 0 and want[5, 33 + 5 + 6].tolist()[0] == 0 and want[7, 33 + 5 + 8].tolist()[2] == 255
    lut = R.magma_lut()
    panel = want[:, 2 * 38:2 * 38 + 33]
    assert np.array_equal(panel[0, 0], lut[0]) and np.array_equal(panel[1, 1], lut[0]) and np.array_equal(panel[2, 2], lut[255])
    unaligned = torch.empty(want.size + 1, dtype=torch.uint8, device=DEV)[1:].view(want.shape)       # a sheet that starts on an odd address
    from samplenerfro_amd import _lib
    import ctypes
    lib = _lib.load()
    dm = [T(m) for m in maps]
    a, b = T(ref), T(test)
    rc = lib.rnerf_errmap_sheet(a.data_ptr(), b.data_ptr(), 29, 33, 4, (ctypes.c_void_p * 4)(*[m.data_ptr() for m in dm]),
                                (ctypes.c_int32 * 4)(*[m.shape[0] for m in dm]), (ctypes.c_int32 * 4)(*[m.shape[1] for m in dm]),
                                unaligned.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and np.array_equal(unaligned.cpu().numpy(), want)


@pytest.mark.parametrize("case", CASES)
def test_bytes_against_the_references_recorded_bytes(fix, device_maps, case):
    from samplenerfro_amd import errmap
    _, _, got = device_maps[case]
    for n in MAPS:
        mine, theirs = indices(errmap.colorize(got[n]).cpu().numpy()), indices(fix[f"bytes_{n}_{case}"])
        differ = mine != theirs
        print(f"{case} {n}: {int(differ.sum())} of {differ.size} indices differ (the reference's float32 against float64: {float(fix[f'share_{n}_{case}']):.4f})")
        assert np.max(np.abs(mine - theirs)) <= 1 and differ.mean() <= 0.01, n


def test_quantize8_is_the_png_a_reader_sees(fix):
    from samplenerfro_amd import errmap
    x = np.concatenate([fix["in_45x70_test"].ravel(), np.arange(256, dtype=np.float32) / np.float32(255), np.linspace(-0.5, 1.5, 4001, dtype=np.float32),
                        np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)])
    got = errmap.quantize8(T(x))
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), R.quantize8(x))
    assert np.array_equal(errmap.quantize8(x.reshape(-1, 1)).cpu().numpy(), R.quantize8(x).reshape(-1, 1))


def test_the_mean_is_bit_stable_and_errors_are_raised():
    from samplenerfro_amd import _lib, errmap, ops
    rng = np.random.default_rng(5)
    a, b = T(rng.uniform(0, 1, (2, 45, 70, 3)).astype(np.float32)), T(rng.uniform(0, 1, (2, 45, 70, 3)).astype(np.float32))
    first = [ops.ssim_summary(a, b)[1].cpu().numpy(), ops.errmap_mse(a, b)[1].cpu().numpy()]
    again = [ops.ssim_summary(a, b)[1].cpu().numpy(), ops.errmap_mse(a, b)[1].cpu().numpy()]
    assert first[0].shape == (2,) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(first, again))
    one = ops.ssim_summary(a[1], b[1])                                # the batch is two independent images
    assert np.array_equal(one[1].cpu().numpy(), first[0][1]) and np.array_equal(one[0].cpu().numpy(), ops.ssim_summary(a, b)[0][1].cpu().numpy())
    img = a[0]
    with pytest.raises(_lib.RnerfError, match="no larger than the image"):
        errmap.sheet(img, img, [torch.zeros((46, 70), device=DEV)])
    with pytest.raises(_lib.RnerfError, match="K must be"):
        errmap.sheet(img, img, [torch.zeros((4, 4), device=DEV)] * 5)
    with pytest.raises(ValueError, match="smaller than the 11 x 11"):
        errmap.error_maps(img[:10], img[:10])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        errmap.error_maps(a, b)
