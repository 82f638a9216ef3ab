"""Profiling helper (not part of the product): time LPIPS (ops.lpips -> rnerf_lpips) on one image pair, value + map.

    python tools/lpips_time.py [--runs 20] [--size 800] [--out f.json]

On a smooth --size x --size image pair already on the device, with seeded random weights (the published ones are not part of this
repository; the time does not depend on the values): (a) ops.lpips(..., return_both=True): five implicit-GEMM convolutions, two pools,
five tap kernels, the value and the map, 14 launches; (b) as a yardstick the same graph through torch's own conv2d / max_pool2d /
interpolate on the same device (the vendor's convolution library in fp32).  HIP events around each call, the workspace and output
allocations of the host layer included.  Two warm-up runs (the library's first call searches for its kernels), then the median of
--runs.  The largest difference between the two maps is printed as a sanity check.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import lpips, ops      # noqa: E402

GEOMETRY = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))      # (stride, padding) of the five convolutions


def median_ms(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(runs + 1)]
    ev[0].record()
    for i in range(runs):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(runs)]
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def random_weights(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    convs, biases, lins = [], [], []
    for co, ci, k in lpips.CONV_SHAPES:
        convs.append(torch.randn((co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5)
        biases.append(torch.randn((co,), generator=g) * 0.1)
        lins.append(torch.rand((1, co, 1, 1), generator=g))
    to = lambda ts: [t.to(dev) for t in ts]
    return lpips.from_tensors(convs, biases, lins, device=dev), to(convs), to(biases), to(lins)


def torch_lpips(a, b, convs, biases, lins):
    """The graph of include/rnerf.h (rnerf_lpips) through torch's operators: -> (map [H, W], value)."""
    H, W = int(a.shape[0]), int(a.shape[1])
    shift = torch.tensor([-0.030, -0.088, -0.188], device=a.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=a.device).view(1, 3, 1, 1)
    x = (2 * torch.stack([a, b]).permute(0, 3, 1, 2) - 1 - shift) / scale
    value, smap = 0, 0
    for l, (stride, pad) in enumerate(GEOMETRY):
        if l in (1, 2):
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, convs[l], biases[l], stride=stride, padding=pad))
        f = x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((f[0:1] - f[1:2]) ** 2, lins[l])
        value = value + d.mean()
        smap = smap + F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)
    return smap[0, 0], value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    dev = torch.device("cuda:0")
    n = a.size
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="ij")
    ref = np.stack([0.5 + 0.4 * np.sin(3 * xx + c) * np.cos(2 * yy - c) for c in range(3)], -1)
    reference = torch.from_numpy(ref.astype(np.float32)).to(dev)
    test = torch.from_numpy(np.clip(ref + 0.03 * rng.standard_normal(ref.shape), 0.0, 1.0).astype(np.float32)).to(dev)
    weights, convs, biases, lins = random_weights(dev)
    with torch.no_grad():
        ours_map, ours_value = ops.lpips(reference, test, weights, return_both=True)
        theirs_map, theirs_value = torch_lpips(reference, test, convs, biases, lins)
        flop = 2 * 2 * sum(co * ci * k * k * h * w for (co, ci, k), (h, w) in zip(lpips.CONV_SHAPES, ops.lpips_layer_shapes(n, n)))
        res = {"tool": "lpips_time", "runs": a.runs, "height": n, "width": n, "conv_gflop": flop / 1e9,
               "value": float(ours_value), "torch_value": float(theirs_value), "max_map_difference": float((ours_map - theirs_map).abs().max()),
               "lpips_ms": median_ms(lambda: ops.lpips(reference, test, weights, return_both=True), a.runs),
               "torch_ms": median_ms(lambda: torch_lpips(reference, test, convs, biases, lins), a.runs)}
    res["conv_tflops"] = flop / (res["lpips_ms"]["median"] * 1e-3) / 1e12
    print(f"{n} x {n}: rnerf_lpips {res['lpips_ms']['median']:.3f} ms ({res['conv_gflop']:.1f} GFLOP in the convolutions, {res['conv_tflops']:.1f} "
          f"TFLOP/s over the whole call), the same graph through torch {res['torch_ms']['median']:.3f} ms; value {res['value']:.6f} vs "
          f"{res['torch_value']:.6f}, largest map difference {res['max_map_difference']:.3e}")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
