"""Profiling helper (not part of the product): time the A/B comparison's two kernels against the same bytes composed with torch operators.

    python tools/compare_time.py [--runs 200] [--size 800] [--out f.json]

On --size x --size inputs already on the device: (a) compare.win_loss with K = 3 and K = 4 maps (rnerf_compare_sheet: one memset, one
launch; the SSIM map is 10 smaller each way, as in compare_views) and (b) compare.strip with N = 3 images and a rectangle
(rnerf_compare_strip: one launch); and for each the same frame composed on the device the way numpy composes it in metric/compare.py
and metric/export.py — boolean masks, float64 colour images, ones panels, concatenation, clip and cast (torch_frame, torch_strip),
with the counts as four sums.  The two forms are checked to give the same bytes and counts before anything is timed.

Timing: HIP events around each call, the host layer's allocations included; three warm-up calls of every form, then --runs rounds that
alternate kernel and torch form so that both see the same machine; the median, minimum and maximum per form.  The bytes a call must
move (maps or images read once, frame written once) over the median give the achieved GB/s.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import compare      # noqa: E402

COLOURS = ((239, 138, 98), (247, 247, 247), (103, 169, 207))      # metric/compare.py:225-227


def torch_frame(maps_a, maps_b, H, W):
    """metric/compare.py:216-236 with torch operators, float64 as numpy has it -> (uint8 [H, K (W + 5), 3], int64 [K, 4])."""
    dev = maps_a[0].device
    # the quotients are numpy's: formed on the device as a tensor divided by the Python scalar 255.0 they did not give numpy's bytes
    # (a division by a scalar carried out as a product with the reciprocal would explain it; not examined)
    ca, ct, cb = (torch.from_numpy(np.array(c, np.float64) / 255.0).to(dev) for c in COLOURS)
    merge, counts = [], []
    for a, b in zip(maps_a, maps_b):
        non = (a - b).abs() < 1e-3
        pos = ~non & (a <= b)
        neg = ~non & (a > b)
        im = ca * pos[..., None].to(torch.float64) + ct * non[..., None].to(torch.float64) + cb * neg[..., None].to(torch.float64)
        pad = torch.ones((H, W, 3), dtype=torch.float64, device=dev)
        pad[:im.shape[0], :im.shape[1]] = im
        merge += [pad, torch.ones((H, 5, 3), dtype=torch.float64, device=dev)]
        n = [pos.sum(), non.sum(), neg.sum()]
        counts.append(torch.stack(n + [a.numel() - n[0] - n[1] - n[2]]))
    return (255.0 * torch.cat(merge, dim=1)).clamp(0, 255).to(torch.uint8), torch.stack(counts)


def torch_strip(images, reference, rect):
    """metric/export.py:92-133 with torch operators, float64 as numpy has it -> uint8 [H, N (W + 5) + W, 3]."""
    dev = reference.device
    H, W = reference.shape[:2]
    x, y, w, h = rect
    weight = torch.full((H, W, 3), 0.5, dtype=torch.float64, device=dev)
    weight[y:y + h, x:x + w] = 1.0
    d255 = torch.tensor(255.0, dtype=torch.float64, device=dev)      # a device tensor as the divisor (see torch_frame)
    white = torch.full((H, 5, 3), 255, dtype=torch.uint8, device=dev)
    parts = []
    for im in images:
        parts += [(((im.to(torch.float64) / d255) * weight + 1.0 * (1 - weight)) * 255.0).clamp(0, 255).to(torch.uint8), white]
    return torch.cat(parts + [reference], dim=1)


def same(what, got, want):
    """The kernel's bytes against the torch form's: anything else is reported with its first places and ends the run."""
    if tuple(got.shape) == tuple(want.shape) and torch.equal(got, want):
        return
    where = torch.nonzero(got != want)[:5].tolist() if tuple(got.shape) == tuple(want.shape) else []
    raise SystemExit(f"{what}: the kernel and the torch form disagree: shapes {tuple(got.shape)} and {tuple(want.shape)}, first places {where}, "
                     f"kernel {[got[tuple(i)].item() for i in where]}, torch {[want[tuple(i)].item() for i in where]}")


def alternate_ms(forms, runs, warmup=3):
    """forms: {name: fn}.  -> {name: {"median", "min", "max"}} in ms, the forms called in turn in every round."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(runs):
        marks = []
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            marks.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in marks:
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    dev = torch.device("cuda:0")
    n = a.size
    rng = np.random.default_rng(0)
    shapes = [(n, n), (n - 10, n - 10), (n, n), (n, n)]                 # psnr, dssim, lpips, flip
    maps_a = [torch.from_numpy(rng.uniform(0, 0.05, s).astype(np.float32)).to(dev) for s in shapes]
    maps_b = [(m + torch.from_numpy((2e-3 * rng.standard_normal(s)).astype(np.float32)).to(dev)) for m, s in zip(maps_a, shapes)]
    images = [torch.from_numpy(rng.integers(0, 256, (n, n, 3), dtype=np.uint8)).to(dev) for _ in range(4)]
    rect = (n // 4, n // 5, n // 2, n // 2)
    res = {"tool": "compare_time", "runs": a.runs, "height": n, "width": n}
    for K in (3, 4):
        ma, mb = (maps_a[:2] + maps_a[3:], maps_b[:2] + maps_b[3:]) if K == 3 else (maps_a, maps_b)
        frame, counts = compare.win_loss(ma, mb, n, n)
        want, want_counts = torch_frame(ma, mb, n, n)
        same(f"win_loss K = {K}", frame, want)
        same(f"win_loss K = {K} counts", counts, want_counts)
        t = alternate_ms({"kernel": lambda: compare.win_loss(ma, mb, n, n), "torch": lambda: torch_frame(ma, mb, n, n)}, a.runs)
        moved = int(frame.numel()) + sum(2 * 4 * int(m.numel()) for m in ma)
        res[f"win_loss_k{K}"] = {"kernel_ms": t["kernel"], "torch_ms": t["torch"], "bytes_moved": moved,
                                 "kernel_gb_per_s": moved / t["kernel"]["median"] * 1e-6, "torch_over_kernel": t["torch"]["median"] / t["kernel"]["median"]}
    strip = compare.strip(images[:3], images[3], rect)
    same("strip N = 3", strip, torch_strip(images[:3], images[3], rect))
    t = alternate_ms({"kernel": lambda: compare.strip(images[:3], images[3], rect), "torch": lambda: torch_strip(images[:3], images[3], rect)}, a.runs)
    moved = int(strip.numel()) + 4 * n * n * 3
    res["strip_n3"] = {"kernel_ms": t["kernel"], "torch_ms": t["torch"], "bytes_moved": moved, "kernel_gb_per_s": moved / t["kernel"]["median"] * 1e-6,
                       "torch_over_kernel": t["torch"]["median"] / t["kernel"]["median"]}
    for key in ("win_loss_k3", "win_loss_k4", "strip_n3"):
        r = res[key]
        print(f"{n} x {n} {key}: kernel {r['kernel_ms']['median']:.4f} ms (min {r['kernel_ms']['min']:.4f}, max {r['kernel_ms']['max']:.4f}; "
              f"{r['bytes_moved']} bytes, {r['kernel_gb_per_s']:.1f} GB/s), torch {r['torch_ms']['median']:.4f} ms (min {r['torch_ms']['min']:.4f}, "
              f"max {r['torch_ms']['max']:.4f}): {r['torch_over_kernel']:.1f} x")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
