"""Host side of the error maps and the comparison sheet (no GPU): tests/helpers/errmap_ref.py against what the reference's own text
recorded in tests/golden/errmap_reference.npz, the committed colour bytes, the byte rules and text formats on cases written by hand,
and the argument checks of the new entry points."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import errmap_ref as R               # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "errmap_reference.npz")
CASES = ("11x11", "29x33", "45x70")
MAPS = ("psnr", "ssim", "flip")


@pytest.fixture(scope="module")
def fix():
    return np.load(FIXTURE)


def test_committed_table_is_the_references_colour_bytes(fix):
    lut = R.magma_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and np.array_equal(lut, fix["lut"])
    assert len({tuple(r) for r in lut}) == 256                      # distinct rows: a colour names its index
    assert tuple(lut[0]) == (0, 0, 3) and tuple(lut[255]) == (251, 252, 191)      # trunc(255 * (0.001462, 0.000466, 0.013866)), ... (0.987053, 0.991438, 0.749504)


def test_committed_table_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    colors = np.asarray(matplotlib.colormaps["magma"].colors, np.float64)
    assert np.array_equal(R.magma_lut(), np.trunc(255.0 * colors).astype(np.uint8))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_magma_table
    assert open(make_magma_table.OUT).read() == make_magma_table.render(matplotlib.colormaps["magma"].colors)


@pytest.mark.parametrize("case", CASES)
def test_helper_colours_the_recorded_maps_bit_for_bit(fix, case):
    for name in MAPS:
        m = fix[f"map_{name}_{case}"]
        assert m.dtype == np.float32
        assert np.array_equal(R.colorize(m), fix[f"bytes_{name}_{case}"]), name       # SSIM: recorded unclipped, coloured clipped — one index


@pytest.mark.parametrize("case", CASES)
def test_helper_maps_are_the_recorded_maps_to_the_recorded_tolerance(fix, case):
    ref, test = fix[f"in_{case}_ref"], fix[f"in_{case}_test"]
    mse_map, mse = R.mse_map(ref, test)
    ssim_map, ssim = R.ssim_summary(ref, test)
    for name, got in (("psnr", mse_map), ("ssim", ssim_map)):
        e_ref = float(fix[f"e_ref_{name}_{case}"])
        assert 0 < e_ref < 1e-5
        assert got.shape == fix[f"map_{name}_{case}"].shape and np.max(np.abs(got - fix[f"map_{name}_{case}"])) <= e_ref * (1 + 1e-9)
    assert ssim_map.shape == (ref.shape[0] - 10, ref.shape[1] - 10)
    assert abs(ssim - float(fix[f"value_ssim_{case}"])) <= float(fix[f"e_ref_ssim_{case}"])
    assert abs(R.psnr_value(mse) - float(fix[f"value_psnr_{case}"])) <= 1e-5 * abs(R.psnr_value(mse)) + 1e-5
    assert float(fix[f"value64_ssim_{case}"]) == ssim and float(fix[f"value64_psnr_{case}"]) == R.psnr_value(mse)


def test_the_fixture_keeps_its_promises(fix):
    assert os.path.getsize(FIXTURE) < 512 * 1024
    for case in CASES:
        for name in MAPS:
            assert float(fix[f"share_{name}_{case}"]) <= 0.01
    blurred = fix["map_ssim_29x33"]
    assert blurred.shape == (19, 23) and blurred.min() < 0.5 and blurred.max() > 0.9       # 69 flat columns, SSIM across its range
    wide = np.concatenate([fix["in_45x70_ref"].ravel(), fix["in_45x70_test"].ravel()])
    assert wide.min() < 0 and wide.max() > 1


def test_byte_rules_by_hand():
    x = np.array([0.0, 0.5, 1.0, -0.25, 1.5, np.nan, 254.999 / 255, np.float32(1 / 255)], np.float32)
    assert R.image_bytes(x).tolist() == [0, 127, 255, 0, 255, 0, 254, 1]
    # 255 * float32(1 / 255) is 1 in double, but an index is formed in float32: the same here, 0.9999999 would truncate to 0
    assert R.map_index(x).tolist() == [0, 127, 255, 0, 255, 0, 254, 1]
    assert R.map_index(np.float32(0.2)).item() == 51 and R.image_bytes(np.float32(0.2)).item() == 51      # 51.000004 in float32, 51.0000007 in double
    b = np.arange(256, dtype=np.uint8)                                # summary.py:233-240: read back / 255 in float32, times 255 in float64
    assert np.array_equal((255.0 * (b.astype(np.float32) / np.float32(255.0)).astype(np.float64)).astype(np.uint8), b)
    assert (R.quantize8(x) * np.float32(255)).tolist() == [0, 127, 255, 0, 255, 0, 254, 1]
    assert R.quantize8(np.float32(0.5)) == np.float32(127) / np.float32(255)


def test_sheet_layout_by_hand():
    lut = R.magma_lut()
    ref, test = np.full((3, 4, 3), 1.0, np.float32), np.zeros((3, 4, 3), np.float32)
    test[0, 0] = [0.5, 2.0, np.nan]
    m = np.array([[0.0, 1.0], [0.5, np.nan]], np.float32)
    s = R.sheet(ref, test, [m])
    assert s.shape == (3, 3 * 9, 3) and s.dtype == np.uint8
    assert (s[:, 0:4] == 255).all() and (s[:, 4:9] == 255).all() and (s[:, 13:18] == 255).all() and (s[:, 22:27] == 255).all()
    assert s[0, 9].tolist() == [127, 255, 0] and not s[:, 9:13].reshape(-1, 3)[1:].any()
    panel = s[:, 18:22]
    assert np.array_equal(panel[:2, :2], lut[[[0, 255], [127, 0]]]) and not panel[2].any() and not panel[:, 2:].any()
    assert R.sheet(ref, test, []).shape == (3, 18, 3)


def test_text_formats_by_hand():
    pytest.importorskip("torch")
    from samplenerfro_amd import errmap
    assert errmap.metric_list_text([31.4159, 9.995], [0.98765, 0.5], [0.01234, 0.25]) == "  0 31.42 0.988 0.012\n  1  9.99 0.500 0.250\n"
    assert errmap.result_text([30.0, 20.0], [0.9, 0.8], [0.1, 0.3]) == " 25.00 0.850 0.200\n"
    assert errmap.MAP_NAMES == MAPS and errmap.GAP == R.GAP == 5
    sheet = np.zeros((4, 5 * 11, 3), np.uint8)
    views = errmap.panels(sheet, [(4, 6), (2, 3), (4, 6)])
    assert [v.shape for v in views] == [(4, 6, 3), (2, 3, 3), (4, 6, 3)]
    with pytest.raises(ValueError, match="panels"):
        errmap.panels(np.zeros((4, 56, 3), np.uint8), [(4, 6)] * 3)


def test_write_error_maps_names_and_slices(tmp_path):
    pytest.importorskip("torch")
    from PIL import Image
    from samplenerfro_amd import errmap
    rng = np.random.default_rng(0)
    sheet = rng.integers(0, 256, (12, 5 * (13 + 5), 3), dtype=np.uint8)
    errmap.write_error_maps(str(tmp_path), 7, sheet, [(12, 13), (2, 3), (12, 13)], "_crop")
    assert sorted(os.listdir(tmp_path)) == ["errmap_crop"]
    assert sorted(os.listdir(tmp_path / "errmap_crop")) == ["flip_007.png", "frame_crop", "psnr_007.png", "ssim_007.png"]
    assert os.listdir(tmp_path / "errmap_crop" / "frame_crop") == ["frame_007.png"]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "errmap_crop" / "frame_crop" / "frame_007.png")), sheet)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "errmap_crop" / "psnr_007.png")), sheet[:, 36:49])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "errmap_crop" / "ssim_007.png")), sheet[:2, 54:57])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "errmap_crop" / "flip_007.png")), sheet[:, 72:85])
    errmap.write_summary_files(str(tmp_path), [31.4159], [0.98765], [0.01234], "_mask")
    assert (tmp_path / "metric_list_mask.txt").read_text() == "  0 31.42 0.988 0.012\n"
    assert (tmp_path / "result_mask.txt").read_text() == " 31.42 0.988 0.012\n"


def test_evaluate_signature():
    pytest.importorskip("torch")
    from samplenerfro_amd import errmap, evaluate, utils
    assert inspect.signature(evaluate.evaluate).parameters["errmap"].default is False
    assert inspect.signature(errmap.error_maps).parameters["pixels_per_degree"].default == utils.FLIP_PPD_SUMMARY


def test_argument_errors_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p = lambda a: ctypes.c_void_p(a)
    A, B, MAP, MEAN, WS, OUT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000      # never dereferenced: every call fails first

    def mse(a=A, b=B, n=1, H=4, W=4, C=3, m=MAP, mean=MEAN, ws=WS):
        return lib.rnerf_errmap_mse(p(a), p(b), n, H, W, C, p(m), p(mean), p(ws), None)

    def ssim(a=A, b=B, n=1, H=16, W=16, C=3, fs=11, sigma=1.5, dr=1.0, m=MAP, mean=MEAN, ws=WS):
        return lib.rnerf_ssim_summary(p(a), p(b), n, H, W, C, fs, sigma, dr, p(m), p(mean), p(ws), None)

    def sheet(a=A, b=B, H=4, W=4, maps=(MAP,), hs=(4,), ws=(4,), out=OUT, K=None):
        K = len(maps) if K is None else K
        n = max(len(maps), 1)
        return lib.rnerf_errmap_sheet(p(a), p(b), H, W, K, (ctypes.c_void_p * n)(*maps), (ctypes.c_int32 * n)(*hs), (ctypes.c_int32 * n)(*ws),
                                      p(out), None)

    cases = [(lambda: mse(a=None), b"null"), (lambda: mse(m=None, mean=None), b"null"), (lambda: mse(H=0), b"H >= 1"), (lambda: mse(C=0), b"C >= 1"),
             (lambda: mse(ws=None), b"workspace"), (lambda: mse(ws=WS + 4), b"aligned"), (lambda: mse(m=A + 16), b"overlaps"),
             (lambda: mse(n=1 << 20, H=1 << 15, W=1 << 15), b"too large"),
             (lambda: ssim(b=None), b"null"), (lambda: ssim(m=None, mean=None), b"null"), (lambda: ssim(H=10), b"smaller than the window"),
             (lambda: ssim(fs=32), b"filter_size"), (lambda: ssim(sigma=0.0), b"filter_sigma"), (lambda: ssim(ws=None), b"workspace"),
             (lambda: ssim(ws=WS + 4), b"aligned"), (lambda: ssim(dr=float("nan")), b"data_range"),
             (lambda: sheet(a=None), b"null"), (lambda: sheet(out=None), b"null"), (lambda: sheet(K=5), b"K must be"), (lambda: sheet(K=-1), b"K must be"),
             (lambda: sheet(maps=(None,)), b"null"), (lambda: sheet(hs=(5,)), b"no larger than the image"), (lambda: sheet(ws=(5,)), b"no larger than the image"),
             (lambda: sheet(hs=(0,)), b"non-empty"), (lambda: sheet(H=0), b"H >= 1"), (lambda: sheet(out=A + 8), b"overlaps"),
             (lambda: sheet(out=B - 8), b"overlaps"), (lambda: sheet(out=MAP + 60), b"overlaps map 0"), (lambda: sheet(H=1 << 15, W=1 << 15), b"2^31")]
    for call, word in cases:
        assert call() == -1, word
        msg = lib.rnerf_last_error()
        assert msg.startswith((b"rnerf_errmap_", b"rnerf_ssim")) and word in msg, (msg, word)
    assert ssim(C=1000) == -3                                        # RNERF_ERR_UNSUPPORTED, as rnerf_ssim
    assert lib.rnerf_ssim_summary_workspace_bytes(1, 16, 16, 1000, 11) == 0 and lib.rnerf_errmap_mse_workspace_bytes(1, 0, 4) == 0
    assert lib.rnerf_errmap_mse_workspace_bytes(2, 800, 800) == 2 * 2500 * 8
    tiles = lib.rnerf_ssim_workspace_bytes(1, 800, 800, 3, 11)
    assert lib.rnerf_ssim_summary_workspace_bytes(1, 800, 800, 3, 11) == tiles + 790 * 790 * 3 * 4
