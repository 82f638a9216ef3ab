"""rnerf_lpips without a GPU: the sizes and argument checks of the C ABI, the weight loader on files written here under both key schemes,
the four-column summary texts, and the float64 / float32 restatement the GPU tests compare against (tests/helpers/lpips_ref.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lpips_ref as R               # noqa: E402

from samplenerfro_amd import _lib   # noqa: E402

P = ctypes.c_void_p


def test_weight_count_and_workspace_query(lib_path):
    lib = _lib.load()
    assert lib.rnerf_lpips_weight_floats() == 2470848 == _lib.LPIPS_WEIGHT_FLOATS == R.WEIGHT_FLOATS
    assert sum(co * ci * k * k + 2 * co for co, ci, k in R.CONV_SHAPES) == 2470848
    for n, H, W in [(1, 30, 31), (1, 31, 30), (1, 30, 30), (0, 64, 64), (-1, 64, 64), (1, 0, 0)]:
        assert lib.rnerf_lpips_workspace_bytes(n, H, W) == 0, (n, H, W)
    lib.rnerf_lpips_workspace_bytes(1, 30, 64)
    assert b"31" in lib.rnerf_last_error()
    small = lib.rnerf_lpips_workspace_bytes(1, 31, 31)
    assert small > 0
    # at least the five taps of both images, the two pooled planes, the d_l and a partial per 64 pixels
    taps = 2 * 4 * (64 * 49 + 192 * 9 + 384 + 256 + 256)
    assert small >= taps + 2 * 4 * (64 * 9 + 192) + 4 * (49 + 9 + 3)
    assert lib.rnerf_lpips_workspace_bytes(2, 31, 31) > small and lib.rnerf_lpips_workspace_bytes(1, 800, 800) > 2 * 4 * 64 * 199 * 199
    # sizes that overflow the kernels' 32-bit indices
    assert lib.rnerf_lpips_workspace_bytes(1, 20000, 20000) == 0 and b"32-bit" in lib.rnerf_last_error()
    assert lib.rnerf_lpips_workspace_bytes(600, 800, 800) == 0
    assert lib.rnerf_lpips_workspace_bytes(1 << 40, 31, 31) == 0


def test_every_argument_check_comes_before_device_work(lib_path):
    lib = _lib.load()
    a, b, w, out, ws = P(1024), P(2048), P(4096), P(8192), P(16384)
    call = lambda *args: lib.rnerf_lpips(*args, None)
    bad = [
        ("null", (None, b, 1, 31, 31, w, out, out, None, ws)),
        ("null", (a, None, 1, 31, 31, w, out, out, None, ws)),
        ("null", (a, b, 1, 31, 31, None, out, out, None, ws)),
        ("nothing to compute", (a, b, 1, 31, 31, w, None, None, None, ws)),
        ("workspace", (a, b, 1, 31, 31, w, out, out, None, None)),
        ("aligned", (a, b, 1, 31, 31, w, out, out, None, P(16388))),
        ("31 x 31", (a, b, 1, 30, 64, w, out, out, None, ws)),
        ("31 x 31", (a, b, 1, 64, 30, w, out, out, None, ws)),
        ("n", (a, b, 0, 64, 64, w, out, out, None, ws)),
        ("32-bit", (a, b, 600, 800, 800, w, out, out, None, ws)),
    ]
    for word, args in bad:
        assert call(*args) == -1, (word, args)
        msg = lib.rnerf_last_error().decode()
        assert msg.startswith("rnerf_lpips") and word in msg, (word, msg)


def alexnet_state_dict(w):
    sd = {}
    for i, cw, cb in zip((0, 3, 6, 8, 10), w["convs"], w["biases"]):
        sd[f"features.{i}.weight"], sd[f"features.{i}.bias"] = cw.clone(), cb.clone()
    sd["classifier.1.weight"], sd["classifier.1.bias"] = torch.zeros(8, 16), torch.zeros(8)
    return sd


def lin_state_dict(w):
    return {f"lin{l}.model.1.weight": t.clone() for l, t in enumerate(w["lins"])}


def full_state_dict(w):
    sd = lin_state_dict(w)
    for s, (i, cw, cb) in enumerate(zip((0, 3, 6, 8, 10), w["convs"], w["biases"])):
        sd[f"net.slice{s + 1}.{i}.weight"], sd[f"net.slice{s + 1}.{i}.bias"] = cw.clone(), cb.clone()
    sd["scaling_layer.shift"], sd["scaling_layer.scale"] = torch.zeros(1, 3, 1, 1), torch.ones(1, 3, 1, 1)
    return sd


def test_the_loader_reads_both_key_schemes(tmp_path):
    from samplenerfro_amd import lpips
    w = R.weight_set()
    want = R.flat(w)
    alex, lin, full = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"), str(tmp_path / "lpips.pth")
    torch.save(alexnet_state_dict(w), alex)
    torch.save(lin_state_dict(w), lin)
    torch.save(full_state_dict(w), full)
    two = lpips.load_weights(alexnet_path=alex, lin_path=lin, device="cpu")
    one = lpips.load_weights(state_dict_path=full, device="cpu")
    direct = lpips.from_tensors(w["convs"], w["biases"], w["lins"], device="cpu")
    for got in (two, one, direct):
        assert got.flat.dtype == torch.float32 and got.flat.shape == (2470848,) and torch.equal(got.flat, want)
        assert got.device == torch.device("cpu")
    # the documented order: conv1.weight first, its bias after it, lin4 last
    assert torch.equal(want[:64 * 3 * 121], w["convs"][0].reshape(-1)) and torch.equal(want[23232:23296], w["biases"][0])
    assert torch.equal(want[-256:], w["lins"][4].reshape(-1))
    squeezed = lpips.from_tensors(w["convs"], w["biases"], [t.reshape(-1) for t in w["lins"]], device="cpu")
    assert torch.equal(squeezed.flat, want)
    with pytest.raises(ValueError):
        lpips.load_weights(alexnet_path=alex, device="cpu")
    with pytest.raises(ValueError):
        lpips.load_weights(alexnet_path=alex, lin_path=lin, state_dict_path=full, device="cpu")


def test_a_missing_or_misshaped_key_raises_and_is_named(tmp_path):
    from samplenerfro_amd import lpips
    w = R.weight_set()
    lin = str(tmp_path / "alex.pth")
    torch.save(lin_state_dict(w), lin)

    def save(sd, name):
        torch.save(sd, str(tmp_path / name))
        return str(tmp_path / name)
    sd = alexnet_state_dict(w)
    del sd["features.6.bias"]
    with pytest.raises(_lib.RnerfError, match=r"features\.6\.bias"):
        lpips.load_weights(alexnet_path=save(sd, "a.pth"), lin_path=lin, device="cpu")
    sd = alexnet_state_dict(w)
    sd["features.3.weight"] = sd["features.3.weight"][:, :, :3, :3].clone()
    with pytest.raises(_lib.RnerfError, match=r"features\.3\.weight.*\(192, 64, 3, 3\)"):
        lpips.load_weights(alexnet_path=save(sd, "b.pth"), lin_path=lin, device="cpu")
    sd = lin_state_dict(w)
    del sd["lin2.model.1.weight"]
    with pytest.raises(_lib.RnerfError, match=r"lin2\.model\.1\.weight"):
        lpips.load_weights(alexnet_path=save(alexnet_state_dict(w), "c.pth"), lin_path=save(sd, "d.pth"), device="cpu")
    sd = full_state_dict(w)
    del sd["net.slice4.8.weight"]
    with pytest.raises(_lib.RnerfError, match=r"net\.slice4\.8\.weight"):
        lpips.load_weights(state_dict_path=save(sd, "e.pth"), device="cpu")
    sd = full_state_dict(w)
    sd["lin0.model.1.weight"] = torch.zeros(1, 63, 1, 1)
    with pytest.raises(_lib.RnerfError, match=r"lin0\.model\.1\.weight"):
        lpips.load_weights(state_dict_path=save(sd, "f.pth"), device="cpu")
    with pytest.raises(_lib.RnerfError, match=r"biases\[1\]"):
        lpips.from_tensors(w["convs"], [w["biases"][0]] * 5, w["lins"], device="cpu")


def test_the_four_column_texts(tmp_path):
    from samplenerfro_amd import errmap
    psnr, ssim, lp, flip = [31.4159, 9.5], [0.98765, 0.5], [0.12345, 0.0625], [0.0456, 0.25]
    assert errmap.MAP_NAMES == ("psnr", "ssim", "flip") and errmap.MAP_NAMES_LPIPS == ("psnr", "ssim", "lpips", "flip")
    assert errmap.metric_list_text(psnr, ssim, flip, lpips_values=lp) == "  0 31.42 0.988 0.123 0.046\n  1  9.50 0.500 0.062 0.250\n"
    assert errmap.result_text(psnr, ssim, flip, lpips_values=lp) == " 20.46 0.744 0.093 0.148\n"
    assert errmap.metric_list_text(psnr, ssim, flip) == "  0 31.42 0.988 0.046\n  1  9.50 0.500 0.250\n"
    assert errmap.result_text(psnr, ssim, flip) == " 20.46 0.744 0.148\n"
    errmap.write_summary_files(str(tmp_path), psnr, ssim, flip, "_crop", lpips_values=lp)
    assert (tmp_path / "metric_list_crop.txt").read_text() == errmap.metric_list_text(psnr, ssim, flip, lp)
    assert (tmp_path / "result_crop.txt").read_text() == " 20.46 0.744 0.093 0.148\n"


def test_write_error_maps_takes_four_shapes(tmp_path):
    from PIL import Image
    from samplenerfro_amd import errmap
    H, W = 6, 7
    sheet = np.arange(H * 6 * (W + 5) * 3, dtype=np.uint32).astype(np.uint8).reshape(H, 6 * (W + 5), 3)
    shapes = [(6, 7), (4, 5), (6, 7), (6, 7)]
    errmap.write_error_maps(str(tmp_path), 3, sheet, shapes)
    names = sorted(os.listdir(tmp_path / "errmap"))
    assert names == ["flip_003.png", "frame", "lpips_003.png", "psnr_003.png", "ssim_003.png"]
    for k, (name, (h, w)) in enumerate(zip(errmap.MAP_NAMES_LPIPS, shapes)):
        x0 = (2 + k) * (W + 5)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "errmap" / f"{name}_003.png")), sheet[:h, x0:x0 + w]), name
    with pytest.raises(ValueError):
        errmap.write_error_maps(str(tmp_path), 3, sheet, shapes + [(6, 7)])


def test_the_metric_files_with_lpips(tmp_path):
    from samplenerfro_amd import evaluate
    evaluate.write_metric_files(str(tmp_path), 7, [30.0], [0.9], None, "_mask", lpips_values=[0.25, 0.5])
    assert sorted(os.listdir(tmp_path)) == ["lpips_7_mask.txt", "lpips_mask.txt", "psnr_mask.txt", "psnrs_7_mask.txt", "ssim_mask.txt", "ssims_7_mask.txt"]
    assert (tmp_path / "lpips_7_mask.txt").read_text() == "0.25 0.5" and (tmp_path / "lpips_mask.txt").read_text() == "0.375"


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------
def test_reference_identical_images_give_zero_and_the_result_is_symmetric():
    c = R.case("31x47")
    value, smap, layers = R.reference(c["img0"], c["img0"], c["weights"])
    assert np.all(value == 0) and np.all(smap == 0) and all(np.all(d == 0) for d in layers)
    v01, m01, l01 = c["ref64"]
    v10, m10, l10 = R.reference(c["img1"], c["img0"], c["weights"])
    assert np.array_equal(v01, v10) and np.array_equal(m01, m10) and all(np.array_equal(x, y) for x, y in zip(l01, l10))
    assert m01.shape == (1, 31, 47) and [d.shape for d in l01] == [(1, 7, 11), (1, 3, 5), (1, 1, 2), (1, 1, 2), (1, 1, 2)]


def test_reference_refuses_30_pixels():
    z = np.zeros((30, 31, 3), np.float32)
    with pytest.raises(ValueError, match="31"):
        R.reference(z, z, R.weight_set())
    with pytest.raises(ValueError, match="31"):
        R.reference(z.transpose(1, 0, 2), z.transpose(1, 0, 2), R.weight_set())
    R.reference(np.zeros((31, 31, 3), np.float32), np.zeros((31, 31, 3), np.float32), R.weight_set())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_cases_are_in_range_and_float32_agrees(name):
    """The GPU tests' bound is max(4 e_ref, 1e-6) with e_ref = |float32 - float64| of this restatement: the values must be large enough
    that the floor is a small share of them, and float32 must agree with float64 to well below it."""
    c = R.case(name)
    v64, m64, l64 = c["ref64"]
    v32, m32, l32 = c["ref32"]
    assert np.all(v64 >= 0.05) and np.all(v64 <= 1.0), v64
    assert np.isfinite(m64).all() and m64.min() >= 0
    assert np.abs(v64 - v32).max() < 1e-5 and np.abs(m64 - m32).max() < 1e-5
    for d64, d32 in zip(l64, l32):
        assert d64.shape == d32.shape and np.abs(d64 - d32).max() < 1e-5
    if name == "dead":
        assert all(np.all(d == 0) for d in l64[2:]) and l64[0].max() > 0 and l64[1].max() > 0
    if name == "31x31":
        assert [d.shape for d in l64] == [(1, 7, 7), (1, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1)]
    if name == "67x93":
        assert [d.shape for d in l64] == [(1, 16, 22), (1, 7, 10), (1, 3, 4), (1, 3, 4), (1, 3, 4)]


def test_layer_shapes_follow_the_reference():
    from samplenerfro_amd import ops
    for name in R.CASES:
        _, H, W, _, _ = R.CASES[name]
        assert ops.lpips_layer_shapes(H, W) == [d.shape[1:] for d in R.case(name)["ref64"][2]]
    assert ops.lpips_layer_shapes(800, 800) == [(199, 199), (99, 99), (49, 49), (49, 49), (49, 49)]
