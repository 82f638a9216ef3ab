"""A numpy restatement of LDR-FLIP (Andersson et al., "FLIP: A Difference Evaluator for Alternating Images", HPG 2020), the yardstick of
rnerf_flip for sizes tests/golden/flip_reference.npz cannot hold.  Written from the paper's formulas with the constants the reference uses
(metric/flip/flip_api.py:134-495); tests/test_flip_host.py pins the float64 form to the vectors the reference's own text computed.

Images are [..., H, W, 3], channels last, sRGB in [0, 1].  `dtype=np.float64` is the exact-arithmetic form; `dtype=np.float32` evaluates
every step in float32 as the reference does (float32 images in, float32 out), which sets the tolerance of the device kernel
(tests/test_gpu_flip.py).  The filters are applied in their full 2-D form (the device uses their separable factors) with the border
replicated."""
import math

import numpy as np

PPD_DEFAULT = (0.7 * 3840 / 0.7) * np.pi / 180          # compute_ldrflip's default: a 0.7 m wide 4K monitor at 0.7 m
PPD_SUMMARY = 0.3 * (400 / 0.5) * np.pi / 180            # metric/summary.py:72-75

# linear RGB -> XYZ (D65), its inverse as the reference states it, and the reference white; all rounded to float32 there
RGB2XYZ = np.array([[10135552 / 24577794, 8788810 / 24577794, 4435075 / 24577794],
                    [2613072 / 12288897, 8788810 / 12288897, 887015 / 12288897],
                    [1425312 / 73733382, 8788810 / 73733382, 70074185 / 73733382]]).astype(np.float32)
XYZ2RGB = np.array([[3.241003275, -1.537398934, -0.498615861],
                    [-0.969224334, 1.875930071, 0.041554224],
                    [0.055639423, -0.204011202, 1.057148933]]).astype(np.float32)
WHITE = np.array([0.950428545, 1.0, 1.088900371]).astype(np.float32)
INV_WHITE = np.array([1.052156925, 1.0, 0.918357670]).astype(np.float32)


def radii(ppd):
    """(spatial radius, feature radius) at `ppd` pixels per degree."""
    return int(np.ceil(3 * np.sqrt(0.04 / (2 * np.pi ** 2)) * ppd)), int(np.ceil(3 * (0.5 * 0.082 * ppd)))


def spatial_filters(ppd):
    """The contrast sensitivity filters of the achromatic, red-green and blue-yellow channels, float64 [2r+1, 2r+1] each, sum 1.
    The squared distance is rounded to float32, as the reference rounds it."""
    r = radii(ppd)[0]
    x, y = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    z = (((x / ppd) ** 2 + (y / ppd) ** 2).astype(np.float32)).astype(np.float64)
    out = []
    for a1, b1, a2, b2 in ((1, 0.0047, 0, 1e-5), (1, 0.0053, 0, 1e-5), (34.1, 0.04, 13.5, 0.025)):
        s = a1 * np.sqrt(np.pi / b1) * np.exp(-np.pi ** 2 * z / b1) + a2 * np.sqrt(np.pi / b2) * np.exp(-np.pi ** 2 * z / b2)
        out.append(s / np.sum(s))
    return out


def feature_filters(ppd):
    """(edge, point) detectors along x, float64 [2r+1, 2r+1]; positive weights sum to 1, negative ones to -1.  Transposed for y."""
    sd = 0.5 * 0.082 * ppd
    r = radii(ppd)[1]
    x, y = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    g = np.exp(-(x ** 2 + y ** 2) / (2 * sd * sd))
    out = []
    for G in (-x * g, (x ** 2 / (sd * sd) - 1) * g):
        neg, pos = -np.sum(G[G < 0]), np.sum(G[G > 0])
        out.append(np.where(G < 0, G / neg, G / pos))
    return out


def correlate(img, kernel):
    """2-D correlation of [..., H, W] with an odd square kernel, border replicated; accumulates in img's dtype."""
    r = kernel.shape[0] // 2
    H, W = img.shape[-2:]
    pad = np.pad(img, [(0, 0)] * (img.ndim - 2) + [(r, r), (r, r)], mode="edge")
    k = kernel.astype(img.dtype)
    acc = np.zeros_like(img)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            acc = acc + k[i, j] * pad[..., i:i + H, j:j + W]
    return acc


def _srgb_to_ycxcz(c, dt):
    lin = np.where(c > dt(0.04045), ((c + dt(0.055)) / dt(1.055)) ** dt(2.4), c / dt(12.92))
    xyz = (lin @ RGB2XYZ.astype(dt).T) * INV_WHITE.astype(dt)
    X, Y, Z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return dt(116) * Y - dt(16), dt(500) * (X - Y), dt(200) * (Y - Z)


def _hunt_lab_of_linear_rgb(rgb, dt):
    xyz = (rgb @ RGB2XYZ.astype(dt).T) * INV_WHITE.astype(dt)
    d = 6 / 29
    f = np.where(xyz > dt(d ** 3), np.cbrt(xyz), dt(1 / (3 * d * d)) * xyz + dt(4 / 29))
    L = dt(116) * f[..., 1] - dt(16)
    a = dt(500) * (f[..., 0] - f[..., 1])
    b = dt(200) * (f[..., 1] - f[..., 2])
    return L, (dt(0.01) * L) * a, (dt(0.01) * L) * b


def _hunt_lab_of_opponent(Y, cx, cz, dt):
    fy = (Y + dt(16)) / dt(116)
    xyz = np.stack([fy + cx / dt(500), fy, fy - cz / dt(200)], -1) * WHITE.astype(dt)
    rgb = np.clip(xyz @ XYZ2RGB.astype(dt).T, dt(0), dt(1))
    return _hunt_lab_of_linear_rgb(rgb, dt)


def _hyab(p, q):
    return np.abs(p[0] - q[0]) + np.sqrt((p[1] - q[1]) ** 2 + (p[2] - q[2]) ** 2)


def cmax(dt=np.float64):
    """The largest HyAB distance the metric maps to 1: Hunt-adjusted green against blue, ^0.7."""
    green = _hunt_lab_of_linear_rgb(np.array([0, 1, 0], dt), dt)
    blue = _hunt_lab_of_linear_rgb(np.array([0, 0, 1], dt), dt)
    return _hyab(green, blue) ** dt(0.7)


def flip(reference, test, pixels_per_degree=PPD_DEFAULT, return_map=True, dtype=np.float64):
    """The FLIP error map [..., H, W] of two [..., H, W, 3] sRGB images (or each image's mean with return_map=False)."""
    dt = dtype
    ppd = float(pixels_per_degree)
    s_a, s_rg, s_by = spatial_filters(ppd)
    edge, point = feature_filters(ppd)
    lab, feat = [], []
    for img in (np.asarray(reference, dt), np.asarray(test, dt)):
        Y, cx, cz = _srgb_to_ycxcz(img, dt)
        lab.append(_hunt_lab_of_opponent(correlate(Y, s_a), correlate(cx, s_rg), correlate(cz, s_by), dt))
        yn = (Y + dt(16)) / dt(116)
        feat.append((np.sqrt(correlate(yn, edge) ** 2 + correlate(yn, edge.T) ** 2),
                     np.sqrt(correlate(yn, point) ** 2 + correlate(yn, point.T) ** 2)))
    cm = cmax(dt)
    pw = _hyab(lab[0], lab[1]) ** dt(0.7)
    pccmax = dt(0.4) * cm
    de_c = np.where(pw < pccmax, (dt(0.95) / pccmax) * pw, dt(0.95) + ((pw - pccmax) / (cm - pccmax)) * dt(1.0 - 0.95))
    de_f = np.maximum(np.abs(feat[0][0] - feat[1][0]), np.abs(feat[1][1] - feat[0][1]))
    de_f = (dt(1 / math.sqrt(2)) * de_f) ** dt(0.5)
    out = de_c ** (dt(1) - de_f)
    return out if return_map else np.mean(out, axis=(-2, -1))
