"""Profiling helper (not part of the product): time the depth visualisations (rnerf_vis_depth, rnerf_vis_normals).

    python tools/vis_time.py [--runs 20] [--size 800] [--out f.json]

Two cases on a smooth --size x --size depth plane with a fractional acc, both already on the device: (a) vis.visualize_suite, what
evaluate(vis_suite=True) adds per view (seven launches: a range reduction and the map for depth and for depth_mod, two moment passes
and the map for the normals); (b) vis.visualize_depth(ignore_frac=0.05), the path that sorts (14 launches: keys, four passes of
histogram and scatter, two over the running sum, one that picks the bounds, the map).  HIP events around each call, the workspace
allocations of the host layer included.  Two warm-up runs, then the median of --runs.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import _lib, vis      # noqa: E402


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
    depth = torch.from_numpy((4 + np.sin(3 * xx) * np.cos(2 * yy) + 0.01 * rng.standard_normal((n, n))).astype(np.float32)).to(dev)
    acc = torch.from_numpy(np.clip(1.2 - (xx ** 2 + yy ** 2), 0, 1).astype(np.float32)).to(dev)
    lib = _lib.load()
    res = {"tool": "vis_time", "runs": a.runs, "height": n, "width": n,
           "suite_launches": 7, "suite_ms": median_ms(lambda: vis.visualize_suite(depth, acc), a.runs),
           "sorted_depth_launches": 14, "sorted_depth_ms": median_ms(lambda: vis.visualize_depth(depth, acc, ignore_frac=0.05), a.runs),
           "sorted_depth_workspace_bytes": int(lib.rnerf_vis_depth_workspace_bytes(n, n, 0.05))}
    print(f"{n} x {n}: visualize_suite median {res['suite_ms']['median']:.3f} ms (7 launches); visualize_depth(ignore_frac=0.05) "
          f"{res['sorted_depth_ms']['median']:.3f} ms (14 launches, workspace {res['sorted_depth_workspace_bytes']} bytes)")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
