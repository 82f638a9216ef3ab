"""Profiling helper (not part of the product): time the bent-path diagnostics on a view of the size users render.

    python tools/path_vis_time.py [--size 800] [--nodes 1536] [--chunks 8192,32768] [--runs 20] [--out f.json]

A smoothed glass ball (n = 1.5) in a 128^3 grid, one --size x --size view of it, --nodes nodes per ray.  Per chunk size:
(a) paths.view_maps for the whole view, and the same loop with HIP events between the march and the summary of every chunk: the two shares;
(b) rnerf_path_summary alone on one chunk's records against the same five maps composed from torch operators on the device (boolean
    mask, sum, argmax, a float64 product and sum over the node axis).  The integer maps must agree exactly and the two float maps to 1e-6
    relative before anything is timed; --runs rounds alternate the two forms.  The kernel reads 32 bytes per node and ray (pd and ior)
    once: those bytes over its median time are the GB/s printed.
Then (c) paths.plot_paths of 256 rays into 4 panels of 512 x 512 (frame="grid": no read-back), HIP events around the call.
Medians, minima and maxima; one JSON line at the end."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import models, ops, paths, synthetic as syn      # noqa: E402
from samplenerfro_amd.utils import Rays                                 # noqa: E402

G, EXT = 128, 1.5


def torch_summary(pd, dr, ior, eps=1e-3):
    """The five maps of rnerf_path_summary from torch operators -> (nodes int32 [3, B], maps float32 [2, B])."""
    N = pd.shape[0]
    g = ior[..., 1:]
    m = torch.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]) > np.float32(eps)
    count = m.sum(0, dtype=torch.int32)
    m8 = m.to(torch.uint8)
    hit = count > 0
    minus = torch.full_like(count, -1)
    first = torch.where(hit, torch.argmax(m8, 0).to(torch.int32), minus)
    last = torch.where(hit, (N - 1 - torch.argmax(torch.flip(m8, [0]), 0)).to(torch.int32), minus)
    d = dr[N - 1, :, :3] - dr[0, :, :3]
    bend = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    e = pd[:-1, :, :3] - pd[1:, :, :3]
    length = torch.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    optical = ((ior[:-1, :, 0] - 1.0).double() * length.double()).sum(0).float()
    return torch.stack([count, first, last]), torch.stack([bend, optical])


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def event_ms(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return stats(out)


def alternate_ms(forms, runs, warmup=2):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(runs):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: stats(v) for name, v in ms.items()}


def split_view(model, rays, chunk):
    """view_maps' loop with events around the march and the summary of every chunk -> (march ms, summary ms) summed over the view."""
    o, v = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    marks = []
    for s in range(0, o.shape[0], chunk):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        pd, dr, ior = paths.march(model, None, Rays(o[s:s + chunk].contiguous(), None, v[s:s + chunk].contiguous(), None))
        e[1].record()
        ops.path_summary(pd, dr, ior)
        e[2].record()
        marks.append(e)
        del pd, dr, ior
    torch.cuda.synchronize()
    return sum(e[0].elapsed_time(e[1]) for e in marks), sum(e[1].elapsed_time(e[2]) for e in marks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--nodes", type=int, default=1536)
    ap.add_argument("--chunks", default="8192,32768")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    dev = torch.device("cuda:0")
    P = 12
    assert a.nodes % P == 0
    raw = torch.from_numpy(syn.scale_ior(syn.sphere_grid(G, EXT, 0.8), 0.5).astype(np.float32)).to(dev)
    grid = ops.grid_prefilter(raw, 5, 1.0)
    model = models.NerfModel(ndim=[G] * 3, nmin=[-EXT] * 3, nmax=[EXT] * 3, grid=grid, num_coarse_samples=a.nodes // P, num_fine_samples=0,
                             num_path_samples=P)
    c2w = np.array([[1, 0, 0, 0], [0, 0, -1, -4.0], [0, 1, 0, 0]], np.float32)          # at y = -4, looking along +y
    H = W = a.size
    o, _, v = ops.generate_rays(c2w, H, W, dev, focal=0.5 * W / math.tan(0.5 * 0.69))
    rays = Rays(o, None, v, None)
    res = {"tool": "path_vis_time", "size": a.size, "nodes": a.nodes, "runs": a.runs, "chunks": {}}
    for chunk in (int(c) for c in a.chunks.split(",")):
        view = event_ms(lambda: paths.view_maps(model, None, rays, chunk=chunk), 3, warmup=1)
        split = [split_view(model, rays, chunk) for _ in range(3)]
        frac = float(paths.view_maps(model, None, rays, chunk=chunk)["refracted"].float().mean())
        # a chunk from the middle rows: its rays cross the ball
        mid = (H // 2) * W
        fl = Rays(o.reshape(-1, 3)[mid:mid + chunk].contiguous(), None, v.reshape(-1, 3)[mid:mid + chunk].contiguous(), None)
        pd, dr, ior = paths.march(model, None, fl)
        nodes, maps = ops.path_summary(pd, dr, ior)
        tn, tm = torch_summary(pd, dr, ior)
        if not torch.equal(nodes, tn):
            raise SystemExit(f"chunk {chunk}: the integer maps of the kernel and of the torch form differ at {int((nodes != tn).sum())} places")
        rel = float(((maps - tm).abs() / tm.abs().clamp_min(1e-30)).max())
        if not rel <= 1e-6:
            raise SystemExit(f"chunk {chunk}: the float maps of the kernel and of the torch form differ by {rel:.3e} relative")
        t = alternate_ms({"kernel": lambda: ops.path_summary(pd, dr, ior), "torch": lambda: torch_summary(pd, dr, ior)}, a.runs)
        moved = 32 * int(pd.shape[0]) * int(pd.shape[1])
        r = {"view_maps_ms": view, "march_ms": float(np.median([s[0] for s in split])), "summary_ms": float(np.median([s[1] for s in split])),
             "refracted_fraction": frac, "kernel_ms": t["kernel"], "torch_ms": t["torch"], "bytes_read": moved,
             "kernel_gb_per_s": moved / t["kernel"]["median"] * 1e-6, "torch_over_kernel": t["torch"]["median"] / t["kernel"]["median"],
             "float_maps_max_rel_diff": rel}
        res["chunks"][str(chunk)] = r
        print(f"{H} x {W} x {a.nodes} nodes, chunk {chunk}: view_maps {view['median']:.1f} ms per view (march {r['march_ms']:.1f}, summary "
              f"{r['summary_ms']:.1f}); summary kernel alone {t['kernel']['median']:.4f} ms (min {t['kernel']['min']:.4f}, max {t['kernel']['max']:.4f}; "
              f"{moved} bytes, {r['kernel_gb_per_s']:.0f} GB/s), torch form {t['torch']['median']:.4f} ms: {r['torch_over_kernel']:.1f} x; "
              f"refracted {frac:.3f}")
        del pd, dr, ior
    # (c) the plot: 256 rays spread over the view's middle rows
    B = 8192
    mid = (H // 2) * W
    fl = Rays(o.reshape(-1, 3)[mid:mid + B].contiguous(), None, v.reshape(-1, 3)[mid:mid + B].contiguous(), None)
    pd, dr, ior = paths.march(model, None, fl)
    sel = np.arange(0, B, B // 256)[:256]
    box = [-EXT] * 3 + [EXT] * 3
    t = event_ms(lambda: paths.plot_paths(pd, ior, sel, size=512, frame="grid", box=box), a.runs)
    res["plot_256_rays_512"] = t
    print(f"plot_paths, 256 rays x {a.nodes} nodes x 4 panels of 512 x 512: {t['median']:.4f} ms (min {t['min']:.4f}, max {t['max']:.4f})")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
