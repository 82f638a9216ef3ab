"""Profiling helper (not part of the product): time the ground-truth renderer on a view of the size users render.

    python tools/scene_time.py [--size 800] [--k 2] [--nodes 1536] [--grid 512] [--runs 5] [--variants] [--out f.json]

A smoothed glass ball (n = 1.5) in a --grid^3 brick table, one --size x --size view of it at supersample --k: (size k)^2 rays of --nodes
nodes.  Reported: the trace (ops.scene_trace over the frame in render_view's chunks of 2^18 rays) in ms and rays/s, the shade
(ops.scene_shade, E = 512) in ms, and in the same run the only other route to the same exit directions: ops.march over the same rays in
chunks of 32768 into one reused pair of record buffers, every record but the last thrown away.  Before anything is timed the trace's
exit directions of the whole frame must equal the march's last records bit for bit.  HIP events, one warm-up, the median of --runs (the
march route: of min(--runs, 3)), the two routes alternating over two rounds; one JSON line at the end.

--variants: load librnerf_experiments.so, which also holds the two four-lanes-per-ray forms the kernel was chosen against
(RNERF_SCENE_VARIANT 4: corners gathered two steps ahead as in march_kernel; 40: no speculation), check that they too give the march's
last records bit for bit and the product kernel's counts, and time them in the same alternation ("trace_variants_ms")."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXT, NEAR, FAR = 1.5, 2.0, 6.0
TRACE_CHUNK, MARCH_CHUNK = 1 << 18, 32768
VARIANTS = {"4": "4 lanes per ray, gathers 2 steps ahead", "40": "4 lanes per ray, no speculation"}


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def event_ms(fn, runs, warmup=1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=1536)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    if a.variants:
        from samplenerfro_amd import _lib, build
        _lib.load(build.LIB_EXPERIMENTS)          # first thing in the process: everything after binds the experiments build
    from samplenerfro_amd import ops, scenes, synthetic as syn
    from samplenerfro_amd._lib import Grid
    dev = torch.device("cuda:0")
    G, N, K = a.grid, a.nodes, a.k
    raw = torch.from_numpy(syn.scale_ior(syn.sphere_grid(G, EXT, 0.8), 0.5).astype(np.float32)).to(dev)
    grid = ops.grid_prefilter(raw, 5, 1.0)
    del raw
    spec = Grid.make([G] * 3, [-EXT] * 3, [EXT] * 3, "bricks")
    table = ops.grid_build_table(grid, spec)
    del grid
    n_inside = scenes.default_n_inside(table, spec)
    fh = fw = a.size * K
    c2w = scenes.pose_spherical(30.0, -30.0, 4.0)
    o, _, v = ops.generate_rays(c2w, fh, fw, dev, focal=0.5 * a.size / math.tan(0.5 * 0.69) * K, pixel_center=True)
    o, v = o.reshape(-1, 3), v.reshape(-1, 3)
    B = int(o.shape[0])
    chunks = [(s, min(B, s + TRACE_CHUNK)) for s in range(0, B, TRACE_CHUNK)]
    exit_dir = torch.empty((B, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((2, B), dtype=torch.int32, device=dev)

    def trace():
        for s, e in chunks:
            x, c = ops.scene_trace(table, spec, o[s:e], v[s:e], NEAR, FAR, N, n_inside=n_inside)
            exit_dir[s:e] = x
            counts[:, s:e] = c

    nb = min(MARCH_CHUNK, B)
    bufs = (torch.empty((N, nb, 4), dtype=torch.float32, device=dev), torch.empty((N, nb, 4), dtype=torch.float32, device=dev))
    last = torch.empty((B, 4), dtype=torch.float32, device=dev)

    def march_route():
        for s in range(0, B, nb):
            e = min(B, s + nb)
            if e - s == nb:
                _, dr, _, _ = ops.march(table, spec, o[s:e], v[s:e], NEAR, FAR, N, out=bufs)
            else:
                _, dr, _, _ = ops.march(table, spec, o[s:e], v[s:e], NEAR, FAR, N)
            last[s:e] = dr[N - 1]

    res = {"tool": "scene_time", "size": a.size, "k": K, "nodes": N, "grid": G, "rays": B, "runs": a.runs, "trace_chunk": TRACE_CHUNK, "march_chunk": nb}
    bits = lambda t: t.contiguous().view(torch.int32)
    march_route()
    torch.cuda.synchronize()
    trace()
    torch.cuda.synchronize()
    if not torch.equal(bits(exit_dir), bits(last)):
        raise SystemExit(f"the trace's exit directions differ from the march's last records at {int((bits(exit_dir) != bits(last)).any(1).sum())} rays")
    print(f"{B} rays x {N} nodes, {G}^3 brick table: exit directions equal the march's last records bit for bit")
    ids = sorted(VARIANTS) if a.variants else []
    product_counts = counts.clone()
    for vid in ids:
        os.environ["RNERF_SCENE_VARIANT"] = vid
        exit_dir.zero_()
        trace()
        torch.cuda.synchronize()
        if not (torch.equal(bits(exit_dir), bits(last)) and torch.equal(counts, product_counts)):
            raise SystemExit(f"variant {vid}: exit directions or counts differ from the march's last records / the product kernel's counts")
    os.environ.pop("RNERF_SCENE_VARIANT", None)
    res["trace_ms"], res["march_route_ms"], res["trace_variants_ms"] = [], [], {v: [] for v in ids}
    for _round in range(2):                               # the routes alternate
        for vid in ids:
            os.environ["RNERF_SCENE_VARIANT"] = vid
            t = event_ms(trace, a.runs)
            res["trace_variants_ms"][vid].append(t)
            print(f"trace [{VARIANTS[vid]}]: {t['median']:.1f} ms (min {t['min']:.1f}, max {t['max']:.1f})")
        os.environ.pop("RNERF_SCENE_VARIANT", None)
        t = event_ms(trace, a.runs)
        res["trace_ms"].append(t)
        print(f"trace: {t['median']:.1f} ms (min {t['min']:.1f}, max {t['max']:.1f}), {B / t['median'] * 1e-3:.2f} M rays/s, "
              f"{B * N / t['median'] * 1e-6:.2f} G node-steps/s")
        m = event_ms(march_route, min(a.runs, 3))
        res["march_route_ms"].append(m)
        print(f"march route (ops.march in chunks of {nb}, records discarded): {m['median']:.1f} ms (min {m['min']:.1f}, max {m['max']:.1f})")
    env = torch.from_numpy(scenes.procedural_env(512, 0)).to(dev)
    step_len = float(np.float32((FAR - NEAR) / (N - 1)))
    s = event_ms(lambda: ops.scene_shade(exit_dir, counts, a.size, a.size, K, env, step_len=step_len, sigma=1.5, albedo=(0.7, 0.2, 0.2)), max(a.runs, 10), warmup=2)
    res["shade_ms"] = s
    print(f"shade ({a.size} x {a.size}, K = {K}, E = 512): {s['median']:.4f} ms (min {s['min']:.4f}, max {s['max']:.4f})")
    res["march_route_over_trace"] = float(np.median([m["median"] for m in res["march_route_ms"]]) / np.median([t["median"] for t in res["trace_ms"]]))
    res["refracted_fraction"] = float((counts[1] > 0).float().mean())
    print(f"march route / trace = {res['march_route_over_trace']:.1f} x; refracted rays {res['refracted_fraction']:.3f}")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh_:
            fh_.write(line + "\n")


if __name__ == "__main__":
    main()
