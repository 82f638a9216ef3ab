"""Profiling helper (not part of the product): time connected-component labelling, statistics and apply at the reference's hull size
(calib/cfg.py: num_voxels 512).

    python tools/components_time.py [--voxels 512 --runs 20 --connectivity 6] [--input hull|noise] [--no-cpu] [--out f.json]

Two inputs: "hull" = a ball plus 300 small floaters (what a carved grid looks like), and "noise" = seeded Bernoulli p = 0.32, just above
the 6-connected site-percolation threshold 0.3116, where components are as ragged as they get (the adversarial input for union-find).
HIP events around rnerf_components_label (three launches), rnerf_components_stats (three memsets and a launch) and rnerf_components_apply
(one launch, on an int32 payload, dropping everything but the largest component).  Two warm-up runs, then the median of --runs.  The time
of one launch alone comes from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/components_time.py --input hull --no-cpu).
The CPU figure is scipy.ndimage.label on the same input on this host, once, when scipy is there.  One JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import _lib, components      # noqa: E402


def hull_input(G, dev, floaters=300):
    t = torch.arange(G, device=dev, dtype=torch.float32) - (G - 1) / 2
    x, y, z = torch.meshgrid(t, t, t, indexing="ij")
    solid = ((x * x + y * y * 1.3 + z * z * 0.8) <= (0.3 * G) ** 2).to(torch.uint8)
    rng = np.random.default_rng(11)
    for _ in range(floaters):
        side = int(rng.integers(1, 5))
        while True:
            c = rng.integers(0, G - side, 3)
            d = c + side / 2 - (G - 1) / 2
            if d[0] ** 2 + d[1] ** 2 * 1.3 + d[2] ** 2 * 0.8 > (0.3 * G + 8) ** 2:
                break
        solid[c[0]:c[0] + side, c[1]:c[1] + side, c[2]:c[2] + side] = 1
    return solid


def noise_input(G, dev, p=0.32):
    gen = torch.Generator(device="cpu"); gen.manual_seed(32)
    return (torch.rand((G, G, G), generator=gen) < p).to(torch.uint8).to(dev)


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
    ap.add_argument("--voxels", type=int, default=512)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--connectivity", type=int, default=6)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--input", choices=("both", "hull", "noise"), default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    G = a.voxels
    n = G ** 3
    dims = (C.c_int32 * 3)(G, G, G)
    st = _lib.current_stream()
    ws = torch.empty(lib.rnerf_components_workspace_bytes(C.byref(dims)) // 4, dtype=torch.int32, device=dev)
    labels = torch.empty((G, G, G), dtype=torch.int32, device=dev)
    size = torch.empty((G, G, G), dtype=torch.int32, device=dev)
    border = torch.empty((G, G, G), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    res = {"tool": "components_time", "voxels": G, "runs": a.runs, "connectivity": a.connectivity}
    for name, make in (("hull", hull_input), ("noise", noise_input)):
        if a.input not in ("both", name):
            continue
        solid = make(G, dev)
        payload = solid.to(torch.int32) * 100

        def do_label():
            _lib.check(lib.rnerf_components_label(_lib.ptr(solid), C.byref(dims), 1, a.connectivity, _lib.ptr(labels), _lib.ptr(ws), st), "label")

        def do_stats():
            _lib.check(lib.rnerf_components_stats(_lib.ptr(labels), C.byref(dims), _lib.ptr(size), _lib.ptr(border), _lib.ptr(counts), st), "stats")

        r = {"solid_voxels": int(solid.sum())}
        r["label_ms"] = median_ms(do_label, a.runs)
        assert int(ws[0]) == 0, "the iteration cap was reached"
        r["stats_ms"] = median_ms(do_stats, a.runs)
        roots, sizes, _ = components.stats(labels)
        keep = torch.zeros(n, dtype=torch.uint8, device=dev)
        keep[roots[:1].long()] = 1

        def do_apply():
            _lib.check(lib.rnerf_components_apply(_lib.ptr(labels), _lib.ptr(keep), 0.0, None, None, 0.0, _lib.ptr(payload), 1, C.byref(dims), st), "apply")

        r["apply_ms"] = median_ms(do_apply, a.runs)
        r["components"], r["largest"] = int(counts[0]), int(sizes[0])
        print(f"{name:6s} {r['solid_voxels']} solid voxels, {r['components']} components, largest {r['largest']}: label {r['label_ms']['median']:.3f} ms, "
              f"stats {r['stats_ms']['median']:.3f} ms, apply {r['apply_ms']['median']:.3f} ms")
        if not a.no_cpu:
            try:
                from scipy import ndimage
            except ImportError:
                ndimage = None
            if ndimage is not None:
                host = solid.cpu().numpy()
                t0 = time.perf_counter()
                _, k = ndimage.label(host, structure=ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[a.connectivity]))
                r["scipy_label_s"] = time.perf_counter() - t0
                assert k == r["components"]
                print(f"       scipy.ndimage.label on this host: {r['scipy_label_s']:.2f} s")
        res[name] = r
        del solid, payload, keep
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
