"""lpips.LPIPS(net='alex'), version 0.1, with normalize=True, restated in torch on the CPU for the tests of rnerf_lpips: the graph of
include/rnerf.h in any dtype, seeded random weights (no published weights are available to the tests), and the cases both GPU test
files share.

reference(img0, img1, weights, dtype) -> (value [n], map [n, H, W], [d_0 .. d_4], d_l: [n, h_l, w_l]), all numpy float64 arrays holding
what the graph gives in `dtype`."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
CONV_SHAPES = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))
CONV_GEOMETRY = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))          # (stride, padding)
MIN_SIZE = 31
WEIGHT_FLOATS = 2470848
# lin_l = LIN_SCALE * |N(0, 1)|: chosen once so that the float64 value of every case below lies in [0.05, 1] (tests/test_lpips_host.py
# asserts it), which keeps the 1e-6 floor of the GPU tests' bound a small share of the value
LIN_SCALE = 0.3


def make_weights(seed=0, conv3_bias=None):
    """Seeded weights as float32 tensors: conv N(0, 2 / fan_in), bias N(0, 0.1^2), lin >= 0 with shape [1, C, 1, 1].  conv3_bias: a
    constant for every bias of conv3 (-1e3 switches taps 2-4 off)."""
    g = torch.Generator().manual_seed(seed)
    convs, biases, lins = [], [], []
    for l, (co, ci, k) in enumerate(CONV_SHAPES):
        fan_in = ci * k * k
        convs.append((torch.randn((co, ci, k, k), generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).float())
        biases.append((torch.randn((co,), generator=g, dtype=torch.float64) * 0.1).float())
        lins.append((torch.randn((1, co, 1, 1), generator=g, dtype=torch.float64).abs() * LIN_SCALE).float())
    if conv3_bias is not None:
        biases[2] = torch.full_like(biases[2], float(conv3_bias))
    return {"convs": convs, "biases": biases, "lins": lins}


def flat(weights) -> torch.Tensor:
    """The flat float32 buffer of include/rnerf.h, built independently of samplenerfro_amd.lpips."""
    parts = []
    for w, b in zip(weights["convs"], weights["biases"]):
        parts += [w.reshape(-1), b.reshape(-1)]
    parts += [l.reshape(-1) for l in weights["lins"]]
    out = torch.cat(parts).float()
    assert out.numel() == WEIGHT_FLOATS
    return out


def features(x, weights, dtype):
    taps = []
    for l, (stride, pad) in enumerate(CONV_GEOMETRY):
        if l in (1, 2):
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, weights["convs"][l].to(dtype), weights["biases"][l].to(dtype), stride=stride, padding=pad))
        taps.append(x)
    return taps


def reference(img0, img1, weights, dtype=torch.float64):
    a, b = (torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float32))) for t in (img0, img1))
    if a.shape != b.shape or a.dim() not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"need two [H, W, 3] or [n, H, W, 3] images, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dim() == 3:
        a, b = a[None], b[None]
    H, W = int(a.shape[1]), int(a.shape[2])
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError(f"LPIPS needs at least {MIN_SIZE} x {MIN_SIZE}, got {H} x {W}")
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)

    def prep(t):
        x = 2 * t.to(dtype).permute(0, 3, 1, 2) - 1
        return (x - shift) / scale

    def unit(f):
        return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)
    with torch.no_grad():
        f0, f1 = features(prep(a), weights, dtype), features(prep(b), weights, dtype)
        layers, value, smap = [], 0, 0
        for l in range(5):
            d = F.conv2d((unit(f0[l]) - unit(f1[l])) ** 2, weights["lins"][l].to(dtype))           # [n, 1, h, w]
            layers.append(d[:, 0].double().numpy())
            value = value + d.mean(dim=(2, 3))[:, 0]
            smap = smap + F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    return value.double().numpy(), smap.double().numpy(), layers


# ---- the cases of the GPU tests -----------------------------------------------------------------------------------------------------
# name -> (n, H, W, kind of pair, conv3 bias of the weight set).  31: every deep tap is 1 x 1 and the bilinear reads a 1 x 1 source;
# 67 x 93: conv1 gives 16 x 22 and both floor pools drop rows / columns; "const": a constant 1.0 image against noise, which shows an input
# scaling folded across conv1's zero padding; "dead": conv3's bias at -1e3, taps 2-4 all zero.
CASES = {
    "31x31": (1, 31, 31, "random", None),
    "31x47": (1, 31, 47, "random", None),
    "67x93": (1, 67, 93, "random", None),
    "batch2": (2, 40, 52, "random", None),
    "const": (1, 67, 93, "const", None),
    "dead": (1, 67, 93, "random", -1e3),
}


@functools.lru_cache(maxsize=None)
def weight_set(conv3_bias=None):
    return make_weights(0, conv3_bias)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(img0, img1: float32 [n, H, W, 3]; weights; ref64, ref32: reference(...) in float64 and float32).  Computed once."""
    n, H, W, kind, conv3_bias = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    img0 = rng.random((n, H, W, 3), dtype=np.float32)
    img1 = rng.random((n, H, W, 3), dtype=np.float32)
    if kind == "const":
        img0 = np.ones_like(img0)
    w = weight_set(conv3_bias)
    return {"img0": img0, "img1": img1, "weights": w, "ref64": reference(img0, img1, w, torch.float64),
            "ref32": reference(img0, img1, w, torch.float32)}
