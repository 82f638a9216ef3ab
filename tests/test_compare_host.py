"""Host side of the A/B comparison (no GPU): tests/helpers/compare_ref.py held to answers derived by hand (metric/compare.py cannot be
run to record a golden file: it imports cv2, lpips and imageio at module level), the file names of compare.write_frames for the three
mask modes, and the argument checks of rnerf_compare_sheet and rnerf_compare_strip."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import compare_ref as R               # noqa: E402

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def test_the_nine_colour_bytes_come_out_of_the_float64_expression():
    c = R.colours()
    assert c.dtype == np.uint8 and c.tolist() == [[239, 138, 98], [247, 247, 247], [103, 169, 207], [0, 0, 0]]
    for v in (239, 138, 98, 247, 103, 169, 207):                     # trunc(clip(255.0 * (v / 255.0))) by hand, component by component
        assert int(np.clip(255.0 * (v / 255.0), 0, 255)) == v
    assert R.save_img_bytes(np.ones((1, 1, 3))).tolist() == [[[255, 255, 255]]]        # the panels and gaps of np.ones


def test_a_two_by_three_map_with_every_class():
    # differences: 0.5 (B lower), 5e-4 (tie), 0.25 (A lower); NaN on the left, NaN on the right, equal infinities (inf - inf = NaN, inf <= inf)
    a = np.array([[0.75, 0.1005, 0.25], [NAN, 0.5, INF]], np.float32)
    b = np.array([[0.25, 0.1, 0.5], [0.5, NAN, INF]], np.float32)
    assert R.classify(a, b).tolist() == [[R.CLASS_B, R.CLASS_TIE, R.CLASS_A], [R.CLASS_NEITHER, R.CLASS_NEITHER, R.CLASS_A]]
    want = [[[103, 169, 207], [247, 247, 247], [239, 138, 98]], [[0, 0, 0], [0, 0, 0], [239, 138, 98]]]
    assert R.colorize(a, b).tolist() == want
    assert R.counts([a], [b]).tolist() == [[2, 1, 1, 2]] and R.counts([a, b], [b, a]).sum(1).tolist() == [6, 6]
    assert R.classify(b, a).tolist() == [[R.CLASS_A, R.CLASS_TIE, R.CLASS_B], [R.CLASS_NEITHER, R.CLASS_NEITHER, R.CLASS_A]]


def test_the_tie_threshold_by_hand():
    t = np.float32(1e-3)
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))
    assert float(below) < 1e-3 < float(t) < float(above)             # float32(1e-3) lies above 1e-3, its neighbour below: no float32 between
    z = np.zeros(7, np.float32)
    d = np.array([0.0, below, t, above, -0.0, INF, -INF], np.float32)
    assert R.classify(z, d).tolist() == [R.CLASS_TIE, R.CLASS_TIE, R.CLASS_A, R.CLASS_A, R.CLASS_TIE, R.CLASS_A, R.CLASS_B]
    assert R.classify(d, z).tolist() == [R.CLASS_TIE, R.CLASS_TIE, R.CLASS_B, R.CLASS_B, R.CLASS_TIE, R.CLASS_B, R.CLASS_A]
    assert R.classify(np.array([INF, -INF, INF], np.float32), np.array([INF, -INF, -INF], np.float32)).tolist() == [R.CLASS_A, R.CLASS_A, R.CLASS_B]


def test_frame_layout_by_hand():
    a = np.array([[0.75, 0.1005, 0.25], [NAN, 0.5, INF]], np.float32)
    b = np.array([[0.25, 0.1, 0.5], [0.5, NAN, INF]], np.float32)
    small = (np.zeros((1, 2), np.float32), np.ones((1, 2), np.float32))
    f = R.frame([a, small[0]], [b, small[1]], 3, 4)
    assert f.shape == (3, 2 * (4 + 5), 3) and f.dtype == np.uint8   # K (W + 5) columns
    assert np.array_equal(f[:2, :3], R.colorize(a, b)) and (f[2, :9] == 255).all() and (f[:, 3:9] == 255).all()
    assert (f[0, 9:11] == [239, 138, 98]).all() and (f[1:, 9:] == 255).all() and (f[:, 11:] == 255).all()
    for K in (1, 3, 4):
        assert R.frame([a] * K, [b] * K, 2, 3).shape == (2, K * 8, 3)


def test_strip_table_and_layout_by_hand():
    t = R.strip_table()
    assert t.shape == (256,) and t.dtype == np.uint8
    assert [int(t[v]) for v in (0, 73, 105, 255)] == [127, 163, 179, 255]              # not (v + 255) // 2 = 127, 164, 180, 255
    assert (73 + 255) // 2 == 164 and (105 + 255) // 2 == 180
    v = np.arange(256)
    assert np.array_equal(np.clip(((v / 255.0) * 1.0 + 1.0 * (1 - 1.0)) * 255.0, 0, 255).astype(np.uint8), v)      # weight 1: the identity
    assert np.abs(t.astype(int) - (v + 255) // 2).max() == 1
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 14
    ref = 255 - img
    s = R.strip([img, img], ref, (1, 0, 2, 1))
    assert s.shape == (2, 2 * (3 + 5) + 3, 3)
    assert np.array_equal(s[:, 16:], ref) and (s[:, 3:8] == 255).all() and (s[:, 11:16] == 255).all()
    assert np.array_equal(s[0, 1:3], img[0, 1:3]) and np.array_equal(s[0, 0], t[img[0, 0]]) and np.array_equal(s[1, :3], t[img[1]])
    assert np.array_equal(s[:, 8:11], s[:, :3])
    assert np.array_equal(R.strip([img], ref), np.hstack([img, np.full((2, 5, 3), 255, np.uint8), ref]))
    assert np.array_equal(R.strip([img], ref, (0, 0, 0, 0)), R.strip([img], ref))


def test_module_constants_panels_and_signature():
    pytest.importorskip("torch")
    from samplenerfro_amd import compare, utils
    assert compare.MAP_NAMES == ("psnr", "dssim", "flip") and compare.MAP_NAMES_LPIPS == ("psnr", "dssim", "lpips", "flip")
    assert compare.GAP == R.GAP == 5
    frame = np.zeros((4, 3 * 11, 3), np.uint8)
    assert [v.shape for v in compare.panels(frame, [(4, 6), (2, 3), (4, 6)])] == [(4, 6, 3), (2, 3, 3), (4, 6, 3)]
    with pytest.raises(ValueError, match="panels"):
        compare.panels(np.zeros((4, 34, 3), np.uint8), [(4, 6)] * 3)
    p = inspect.signature(compare.compare_views).parameters
    assert p["pixels_per_degree"].default == utils.FLIP_PPD_SUMMARY and p["name_b"].default == "b" and p["lpips"].default is None
    assert p["save_output"].default is False and p["strips"].default is False and p["masks"].default is None
    assert inspect.signature(compare.win_loss).parameters["counts"].default is True


@pytest.mark.parametrize("mode,suffix", [(None, ""), ("mask", "_mask"), ("crop", "_crop"), ("mask_crop", "_mask")])
def test_file_names_and_suffixes(tmp_path, mode, suffix):
    pytest.importorskip("torch")
    from PIL import Image
    from samplenerfro_amd import compare, evaluate
    assert evaluate.mask_suffix(mode) == suffix                      # compare.py:153 parses like summary.py:165
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (12, 3 * (13 + 5), 3), dtype=np.uint8)
    strip = rng.integers(0, 256, (12, 2 * 18 + 13, 3), dtype=np.uint8)
    compare.write_frames(str(tmp_path), 7, frame, [(12, 13), (2, 3), (12, 13)], "half", suffix, strip)
    top = tmp_path / f"compare_half{suffix}"
    assert os.listdir(tmp_path) == [top.name]
    assert sorted(os.listdir(top)) == sorted(["psnr_007.png", "dssim_007.png", "flip_007.png", "frame" + suffix, "strip" + suffix])
    assert os.listdir(top / ("frame" + suffix)) == ["frame_007.png"] and os.listdir(top / ("strip" + suffix)) == ["strip_007.png"]
    assert np.array_equal(np.asarray(Image.open(top / ("frame" + suffix) / "frame_007.png")), frame)
    assert np.array_equal(np.asarray(Image.open(top / ("strip" + suffix) / "strip_007.png")), strip)
    assert np.array_equal(np.asarray(Image.open(top / "psnr_007.png")), frame[:, 0:13])
    assert np.array_equal(np.asarray(Image.open(top / "dssim_007.png")), frame[:2, 18:21])
    assert np.array_equal(np.asarray(Image.open(top / "flip_007.png")), frame[:, 36:49])


def test_four_maps_write_the_lpips_panel_and_load_preds_sorts(tmp_path):
    pytest.importorskip("torch")
    from PIL import Image
    from samplenerfro_amd import compare
    frame = np.random.default_rng(1).integers(0, 256, (6, 4 * (7 + 5), 3), dtype=np.uint8)
    compare.write_frames(str(tmp_path), 0, frame, [(6, 7), (2, 3), (6, 7), (6, 7)])
    assert sorted(os.listdir(tmp_path / "compare_b")) == ["dssim_000.png", "flip_000.png", "frame", "lpips_000.png", "psnr_000.png"]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "compare_b" / "lpips_000.png")), frame[:, 24:31])
    with pytest.raises(ValueError, match="write_frames"):
        compare.write_frames(str(tmp_path), 0, frame, [(6, 7)] * 2)
    preds = tmp_path / "test_preds"
    preds.mkdir()
    for name, value in (("001.png", 1), ("000.png", 0), ("disp_000.png", 9), ("0002.png", 9), ("010.png", 10)):
        Image.fromarray(np.full((2, 3, 4 if value == 10 else 3), value, np.uint8)).save(preds / name)
    got = list(compare.load_preds(str(preds)))
    assert [g.shape for g in got] == [(2, 3, 3)] * 3 and [int(g[0, 0, 0]) for g in got] == [0, 1, 10] and got[0].dtype == np.uint8


def test_argument_errors_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p = lambda a: ctypes.c_void_p(a)
    A, B, OUT, CNT, IMG, REF = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000      # never dereferenced: every call fails first

    def sheet(H=4, W=4, a=(A,), b=(B,), hs=(4,), ws=(4,), out=OUT, counts=CNT, K=None, arrays=True):
        K = len(a) if K is None else K
        n = max(len(a), 1)
        arr = lambda t, vals: (t * n)(*vals) if arrays else None
        return lib.rnerf_compare_sheet(H, W, K, arr(ctypes.c_void_p, a), arr(ctypes.c_void_p, b), arr(ctypes.c_int32, hs), arr(ctypes.c_int32, ws),
                                       p(out), p(counts), None)

    def strip(images=(IMG,), N=None, ref=REF, H=4, W=6, rect=(0, 0, 0, 0), out=OUT, array=True):
        N = len(images) if N is None else N
        arr = (ctypes.c_void_p * max(len(images), 1))(*images) if array else None
        return lib.rnerf_compare_strip(arr, N, p(ref), H, W, *rect, p(out), None)

    cases = [(lambda: sheet(K=0), b"K must be"), (lambda: sheet(K=5), b"K must be"), (lambda: sheet(a=(A,) * 5, b=(B,) * 5, hs=(4,) * 5, ws=(4,) * 5), b"K must be"),
             (lambda: sheet(hs=(5,)), b"no larger than the image"), (lambda: sheet(ws=(5,)), b"no larger than the image"),
             (lambda: sheet(hs=(0,)), b"non-empty"), (lambda: sheet(ws=(0,)), b"non-empty"), (lambda: sheet(H=0), b"H >= 1"), (lambda: sheet(W=0), b"W >= 1"),
             (lambda: sheet(arrays=False), b"null"), (lambda: sheet(out=None), b"null"), (lambda: sheet(a=(None,)), b"null pointer (map 0)"),
             (lambda: sheet(b=(A, None), a=(A, B), hs=(4, 4), ws=(4, 4)), b"null pointer (map 1)"),
             (lambda: sheet(H=1 << 15, W=1 << 15), b"2^31"), (lambda: sheet(out=A + 60), b"out overlaps map 0"), (lambda: sheet(out=B - 8), b"out overlaps map 0"),
             (lambda: sheet(counts=B + 56), b"counts overlaps map 0"), (lambda: sheet(counts=OUT + 8), b"out overlaps counts"),
             (lambda: sheet(counts=CNT + 4), b"aligned"),
             (lambda: strip(N=0), b"N must be"), (lambda: strip(images=(IMG,) * 5), b"N must be"), (lambda: strip(N=5), b"N must be"),
             (lambda: strip(array=False), b"null"), (lambda: strip(ref=None), b"null"), (lambda: strip(out=None), b"null"),
             (lambda: strip(images=(IMG, None)), b"null pointer (image 1)"), (lambda: strip(H=0), b"H >= 1"),
             (lambda: strip(rect=(5, 0, 2, 1)), b"inside the image"), (lambda: strip(rect=(0, 3, 1, 2)), b"inside the image"),
             (lambda: strip(rect=(-1, 0, 2, 2)), b"inside the image"), (lambda: strip(rect=(0, 0, 7, 1)), b"inside the image"),
             (lambda: strip(rect=(0, 0, -1, 2)), b"inside the image"), (lambda: strip(rect=(0, 0, 1 << 31 - 1, 2)), b"inside the image"),
             (lambda: strip(out=IMG + 8), b"out overlaps image 0"), (lambda: strip(out=REF - 8), b"out overlaps the reference"),
             (lambda: strip(H=1 << 15, W=1 << 15), b"2^31")]
    for call, word in cases:
        assert call() == -1, word
        msg = lib.rnerf_last_error()
        assert msg.startswith(b"rnerf_compare_") and word in msg, (msg, word)
