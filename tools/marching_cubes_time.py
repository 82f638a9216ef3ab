"""Profiling helper (not part of the product): time device marching cubes (rnerf_marching_cubes_*, csrc/mcubes.hip).

    python tools/marching_cubes_time.py [--runs 10] [--out f.json]

Two fields: 512^3 hull-like binary data (a bumpy blob as count / V > threshold gives it, iso 0.5: the setting of
calib/make_visual_hull.py:148) and a smooth 257^3 float field (the lattice of extract_mesh.py at its default resolution 256).  HIP events
around (a) rnerf_marching_cubes_count (the count and the scan launch; the C ABI does not launch them apart — a kernel trace splits them),
(b) the vertex launch alone (faces_capacity 0), (c) the triangle launch alone (verts_capacity 0, after (b)), (d) both calls as
marching_cubes() issues them, (e) marching_cubes() itself, with its allocations and its 16-byte readback.  Two warm-up runs, then the
median of --runs.  Beside them the floor of the shape at the measured HBM copy rate of 6.3 TB/s: the field read once, vbase written and
read once, the outputs written once.  One JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import _lib, marching_cubes      # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def waves(G, dev, seed, n=5, min_wavelength=24.0):
    g = torch.Generator().manual_seed(seed)
    ax = torch.arange(G, dtype=torch.float32, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    out = torch.zeros((G, G, G), dtype=torch.float32, device=dev)
    for _ in range(n):
        k = torch.randn(3, generator=g)
        k = k * (2 * np.pi / (min_wavelength * (1 + 2 * float(torch.rand(1, generator=g))) * float(k.norm())))
        out += torch.sin(x * float(k[0]) + y * float(k[1]) + z * float(k[2]) + 6.283 * float(torch.rand(1, generator=g)))
    return out, (x, y, z)


def fields(dev):
    w, (x, y, z) = waves(512, dev, 1)
    r = torch.sqrt((x - 255.5) ** 2 + (y - 255.5) ** 2 + (z - 255.5) ** 2)
    hull = ((w * 12.0 + (170.0 - r)) > 0).to(torch.float32)
    del w, x, y, z, r
    smooth, (x, y, z) = waves(257, dev, 2)
    r = torch.sqrt((x - 128) ** 2 + (y - 128) ** 2 + (z - 128) ** 2)
    smooth = smooth + (100.0 - r) / 20.0
    return (("hull_like_binary_512", hull, 0.5), ("smooth_257", smooth.contiguous(), 0.0))


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
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    assert a.runs >= 10, "the median is taken over at least 10 runs"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = _lib.current_stream()
    res = {"tool": "marching_cubes_time", "runs": a.runs, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "fields": {}}
    for name, field, iso in fields(dev):
        dims = (C.c_int32 * 3)(*field.shape)
        d = C.byref(dims)
        N = field.numel()
        ws = torch.empty(lib.rnerf_marching_cubes_workspace_bytes(d) // 8 + 1, dtype=torch.int64, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)

        def count():
            _lib.check(lib.rnerf_marching_cubes_count(_lib.ptr(field), d, iso, _lib.ptr(ws), _lib.ptr(totals), st), "count")

        count()
        V, F = totals.tolist()
        verts = torch.empty((V, 3), dtype=torch.float64, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)

        def emit(cap_v, cap_f):
            _lib.check(lib.rnerf_marching_cubes_emit(_lib.ptr(field), d, iso, _lib.ptr(ws), _lib.ptr(verts), cap_v, _lib.ptr(faces), cap_f,
                                                     _lib.ptr(overflow), st), "emit")

        def both():
            count()
            emit(V, F)

        r = {"dims": list(field.shape), "iso": iso, "vertices": V, "triangles": F,
             "count_and_scan_launches_ms": median_ms(count, a.runs),
             "vertex_launch_ms": median_ms(lambda: emit(V, 0), a.runs),
             "triangle_launch_ms": median_ms(lambda: emit(0, F), a.runs),
             "count_and_emit_calls_ms": median_ms(both, a.runs),
             "marching_cubes_python_ms": median_ms(lambda: marching_cubes.marching_cubes(field, iso), a.runs)}
        assert int(overflow.item()) == 0
        floor_bytes = 4 * N + 2 * 4 * N + 24 * V + 12 * F
        r["floor"] = {"bytes": floor_bytes, "ms": floor_bytes / HBM_BYTES_PER_S * 1e3,
                      "what": "field read once, vbase written and read once, vertices and triangles written once"}
        res["fields"][name] = r
        print(f"{name}: {V} vertices, {F} triangles; floor {r['floor']['ms']:.3f} ms ({floor_bytes / 1e6:.1f} MB)")
        for k, v in r.items():
            if k.endswith("_ms"):
                print(f"  {k:32s} median {v['median']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f})")
        del ws, verts, faces
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
