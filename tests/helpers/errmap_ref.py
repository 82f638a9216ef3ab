"""metric/summary.py's error maps and comparison sheet restated in numpy (host only): the float64 maps (summary.py:49-61 over
metric/ssim/ssim.py:45-133), the byte rules of save_img / save_err (:40-45) and the sheet layout of :231-240, which live inside main()
there and cannot be executed alone.  tests/golden/errmap_reference.npz holds what the reference's own text gives on the same inputs;
tests/test_errmap_host.py holds this file to it."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_H = os.path.join(HERE, "..", "..", "samplenerfro_amd", "csrc", "magma_table.h")
GAP = 5
WIN_SIZE, WIN_SIGMA = 11, 1.5


def magma_lut(path=TABLE_H):
    """The committed colour bytes, uint8 [256, 3], parsed from csrc/magma_table.h."""
    text = open(path).read()
    body = text[text.index("{", text.index("#define RNERF_MAGMA_TABLE")) + 1:text.rindex("}")]
    vals = [int(v) for v in re.findall(r"\d+", body)]
    assert len(vals) == 768 and max(vals) <= 255
    return np.array(vals, np.uint8).reshape(256, 3)


def gauss_window(size=WIN_SIZE, sigma=WIN_SIGMA):
    """_fspecial_gauss_1d (ssim.py:20-24) in float64."""
    c = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-(c ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _blur_valid(x, win):
    """gaussian_filter (ssim.py:39-42) on [H, W, C]: the window along W, then along H, "valid"."""
    n = win.shape[0]
    H, W = x.shape[:2]
    h = sum(win[k] * x[:, k:k + W - n + 1] for k in range(n))
    return sum(win[k] * h[k:k + H - n + 1] for k in range(n))


def mse_map(ref, test):
    """summary.py:51,54 in float64 -> (map [H, W], mse)."""
    d = (np.asarray(ref, np.float64) - np.asarray(test, np.float64)) ** 2
    return d.mean(-1), float(d.mean())


def psnr_value(mse):
    """summary.py:52."""
    return float(-20.0 * np.log10(np.sqrt(mse)))


def ssim_summary(ref, test, data_range=1.0):
    """ssim.py:59-86,127-129 in float64 on [H, W, C] -> (map [H-10, W-10] the channel mean, unclipped; value)."""
    X, Y = np.asarray(ref, np.float64), np.asarray(test, np.float64)
    win = gauss_window()
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = _blur_valid(X, win), _blur_valid(Y, win)
    s11 = _blur_valid(X * X, win) - mu1 * mu1
    s22 = _blur_valid(Y * Y, win) - mu2 * mu2
    s12 = _blur_valid(X * Y, win) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s11 + s22 + C2))
    return m.mean(-1), float(m.mean())


def image_bytes(img):
    """save_img (summary.py:40-41) on the float64 hstack: trunc(clip(255.0 * float64(x), 0, 255)); NaN -> 0 (the documented deviation)."""
    v = 255.0 * np.asarray(img, np.float32).astype(np.float64)
    return np.where(np.isnan(v), 0.0, np.clip(v, 0, 255)).astype(np.uint8)


def map_index(m):
    """save_err's index (summary.py:44 and index2color's astype(int)): trunc(clip(255.0 * float32(v), 0, 255)) in float32; NaN -> 0."""
    v = np.float32(255.0) * np.asarray(m, np.float32)
    assert v.dtype == np.float32
    return np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(255))).astype(np.int64)


def colorize(m, lut=None):
    """save_err -> uint8 [h, w, 3]."""
    lut = magma_lut() if lut is None else lut
    return lut[map_index(m)]


def quantize8(img):
    """The reader's view of utils.save_img's PNG: trunc(clip(x, 0, 1) * 255) / 255 in float32; NaN -> 0."""
    x = np.asarray(img, np.float32)
    u = (np.clip(np.where(np.isnan(x), np.float32(0), x), np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint8)
    return u.astype(np.float32) / np.float32(255.0)


def sheet(ref, test, maps, lut=None):
    """summary.py:231-240 -> uint8 [H, (2 + K)(W + 5), 3].  The PNG round trip of :233 (bytes / 255 in float32, times 255 in float64,
    truncated) is the identity on all 256 byte values (tests/test_errmap_host.py), so the panels carry the colour bytes."""
    H, W = np.shape(ref)[:2]
    white = np.full((H, GAP, 3), 255, np.uint8)
    merge = [image_bytes(ref), white, image_bytes(test), white]
    for m in maps:
        im = colorize(m, lut)
        pad = np.zeros((H, W, 3), np.uint8)
        pad[:im.shape[0], :im.shape[1]] = im
        merge += [pad, white]
    return np.hstack(merge)
