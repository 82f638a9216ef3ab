"""Profiling helper (not part of the product): time visual-hull carving at the reference's own setting (calib/cfg.py: num_voxels 512).

    python tools/visual_hull_time.py [--voxels 512 --views 100 --height 1080 --width 1920 --runs 10] [--out f.json]

Synthetic scene: cameras on an orbit around the box, elliptical masks.  HIP events around (a) rnerf_visual_hull_pack alone, (b)
rnerf_visual_hull_count on the packed bits alone (masks == NULL), (c) rnerf_visual_hull_finalize alone, (d) count (packing included) +
finalize, the sequence a caller runs.  Two warm-up runs, then the median of --runs.  Reported: ms in total and per view, voxel-views per
second, the mask / packed / count / grid bytes moved.

The CPU figure is NOT a measurement of the reference at 512^3: it is the numpy loop of tests/helpers/visual_hull_ref.py for one view at
G = 128 on this host, scaled by 64 (= 512^3 / 128^3), labelled as such.  One JSON line at the end."""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from samplenerfro_amd import _lib, visual_hull      # noqa: E402


def look_at(pos, target):
    f = (target - pos) / np.linalg.norm(target - pos)
    r = np.cross(f, [0.0, 0.0, 1.0]); r /= np.linalg.norm(r)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = r, np.cross(f, r), f, pos
    return T


def scene(V, H, W, dev):
    """cam_mat, transforms [V,4,4], masks uint8 [V,H,W] on the device: an ellipsoid of radius ~0.45 seen from an orbit of radius 3."""
    f = 1.2 * W
    cam = np.array([[f, 0, W / 2 - 0.3], [0, f, H / 2 + 0.2], [0, 0, 1.0]])
    rng = np.random.default_rng(7)
    Ts = []
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    masks = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    for v in range(V):
        az, el = 2 * np.pi * v / V, rng.uniform(-0.4, 0.6)
        pos = 3.0 * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        T = look_at(pos, rng.uniform(-0.05, 0.05, 3))
        Ts.append(T)
        pc = T[:3, :3].T @ (-pos)
        u0, v0 = f * pc[0] / pc[2] + cam[0, 2], f * pc[1] / pc[2] + cam[1, 2]
        rx, ry = f * 0.45 / pc[2], f * 0.35 / pc[2]
        masks[v] = ((((xx - u0) / rx) ** 2 + ((yy - v0) / ry) ** 2) <= 1.0).to(torch.uint8) * 255
    return cam, np.stack(Ts), masks


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
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--cpu-voxels", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    assert a.runs >= 10 or a.voxels < 512, "the median is taken over at least 10 runs"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    G, V, H, W = a.voxels, a.views, a.height, a.width
    cam, Ts, masks = scene(V, H, W, dev)
    pv = torch.from_numpy(visual_hull.projection_matrices(cam, Ts)).to(dev)
    spec = _lib.Grid.make([G] * 3, [-1.0] * 3, [1.0] * 3)
    ws = torch.empty(lib.rnerf_visual_hull_workspace_bytes(V, H, W) // 4, dtype=torch.int32, device=dev)
    count = torch.empty((G, G, G), dtype=torch.int32, device=dev)
    out = torch.empty((G, G, G), dtype=torch.float32, device=dev)
    st = _lib.current_stream()
    g = C.byref(spec)

    def pack():
        _lib.check(lib.rnerf_visual_hull_pack(_lib.ptr(masks), V, H, W, _lib.ptr(ws), st), "pack")

    def count_only():
        _lib.check(lib.rnerf_visual_hull_count(None, V, H, W, _lib.ptr(pv), g, 0, _lib.ptr(count), _lib.ptr(ws), st), "count")

    def finalize():
        _lib.check(lib.rnerf_visual_hull_finalize(_lib.ptr(count), g, V, 0.9, 1.33, 1.0, _lib.ptr(out), st), "finalize")

    def whole():
        _lib.check(lib.rnerf_visual_hull_count(_lib.ptr(masks), V, H, W, _lib.ptr(pv), g, 0, _lib.ptr(count), _lib.ptr(ws), st), "count")
        finalize()

    res = {"tool": "visual_hull_time", "voxels": G, "views": V, "height": H, "width": W, "runs": a.runs,
           "bytes": {"masks_read": V * H * W, "packed_bits": int(ws.numel()) * 4, "count_written": 4 * G ** 3, "grid_written": 4 * G ** 3}}
    vv = float(G) ** 3 * V
    for name, fn in (("pack", pack), ("count", count_only), ("finalize", finalize), ("count_with_pack_and_finalize", whole)):
        med, lo, hi = median_ms(fn, a.runs)
        res[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        print(f"{name:30s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f})")
    tot = res["count_with_pack_and_finalize_ms"]["median"]
    res["ms_per_view"] = tot / V
    res["voxel_views_per_s"] = vv / (tot * 1e-3)
    res["count_kernel_voxel_views_per_s"] = vv / (res["count_ms"]["median"] * 1e-3)
    res["pack_GB_per_s"] = V * H * W / (res["pack_ms"]["median"] * 1e-3) / 1e9
    res["hull_voxels"] = int((out > 1.0).sum())
    res["distinct_counts"] = int(torch.unique(count).numel())
    print(f"total {tot:.3f} ms = {tot / V:.4f} ms per view, {res['voxel_views_per_s']:.4g} voxel-views/s; hull {res['hull_voxels']} voxels, "
          f"{res['distinct_counts']} distinct counts")

    # the CPU figure: one view of the numpy loop at a smaller grid, scaled by the voxel ratio — not a measurement at --voxels
    import visual_hull_ref
    Gc = a.cpu_voxels
    m0 = masks[0].cpu().numpy()
    t0 = time.perf_counter()
    visual_hull_ref.counts([m0], cam, Ts[:1], Gc, [-1.0] * 3, [1.0] * 3)
    dt = time.perf_counter() - t0
    scale = (G / Gc) ** 3
    res["cpu_numpy_loop"] = {"voxels": Gc, "views": 1, "seconds": dt, "scaled_by": scale, "scaled_seconds_per_view": dt * scale,
                             "note": "tests/helpers/visual_hull_ref.py on this host, scaled by the voxel ratio; not the reference at full size"}
    print(f"CPU (numpy loop, one view, G = {Gc}): {dt:.3f} s; x {scale:g} = {dt * scale:.1f} s per view at G = {G} (a scaled figure)")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
