"""Profiling helper (not part of the product): time the mesh rasteriser and the mask dilation (rnerf_mesh_depth, rnerf_mask_dilate).

    python tools/mesh_mask_time.py [--runs 10] [--ball 512] [--out f.json]

Two cases: (a) the example scene's OBJ (tests/golden/example_obj.npz, 55 340 faces) from the example camera at 800 x 800; (b) the
marching-cubes mesh of a ball of radius 0.3 G in a G^3 grid (--ball, default 512; the face count is reported) from a Blender-model
camera at 1080 x 1920 that sees all of it.  HIP events around rnerf_mesh_depth alone (all five launches, the mesh already on the
device, the workspace reused) and around rnerf_mask_dilate with the 35 x 35 box alone.  Two warm-up runs, then the median of --runs.
One JSON line at the end."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from samplenerfro_amd import _lib, marching_cubes, mesh_mask      # noqa: E402


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


def time_case(name, v, f, c2w, H, W, focal, runs):
    lib = _lib.load()
    dev = v.device
    V, F = int(v.shape[0]), int(f.shape[0])
    ws = torch.empty(lib.rnerf_mesh_depth_workspace_bytes(V, F, H, W) // 8, dtype=torch.int64, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    tri = torch.empty((H, W), dtype=torch.int32, device=dev)
    hits = torch.empty((H, W), dtype=torch.int32, device=dev)
    skipped = torch.empty(1, dtype=torch.int64, device=dev)
    cam = np.ascontiguousarray(np.asarray(c2w, np.float32)[:3, :4])
    st = _lib.current_stream()

    def raster():
        _lib.check(lib.rnerf_mesh_depth(_lib.ptr(v), V, _lib.ptr(f), F, cam.ctypes.data, 0, focal, focal, W * 0.5, H * 0.5, 0.5, H, W, 0.1, 100.0,
                                        _lib.ptr(depth), _lib.ptr(tri), _lib.ptr(hits), _lib.ptr(skipped), _lib.ptr(ws), st), "rnerf_mesh_depth")

    res = {"faces": F, "verts": V, "height": H, "width": W, "workspace_bytes": int(ws.numel()) * 8, "mesh_depth_ms": median_ms(raster, runs)}
    mask = (depth != 0).to(torch.uint8)
    out = torch.empty_like(mask)
    bbox = torch.empty(4, dtype=torch.int32, device=dev)
    dws = torch.empty((lib.rnerf_mask_dilate_workspace_bytes(H, W) + 7) // 8, dtype=torch.int64, device=dev)

    def dilate():
        _lib.check(lib.rnerf_mask_dilate(_lib.ptr(mask), H, W, 35, 35, _lib.ptr(out), _lib.ptr(bbox), _lib.ptr(dws), st), "rnerf_mask_dilate")

    res["mask_dilate_35_ms"] = median_ms(dilate, runs)
    res["covered_pixels"] = int(mask.sum())
    res["odd_hit_pixels"] = int((hits % 2 == 1).sum())
    res["skipped"] = int(skipped.cpu())
    res["bbox"] = [int(x) for x in bbox.cpu()]
    print(f"{name:12s} {F:8d} faces at {H} x {W}: rnerf_mesh_depth median {res['mesh_depth_ms']['median']:.3f} ms, 35 x 35 dilation "
          f"{res['mask_dilate_35_ms']['median']:.3f} ms; {res['covered_pixels']} covered pixels, {res['odd_hit_pixels']} with an odd hit count")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--ball", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    dev = torch.device("cuda:0")
    import cases
    res = {"tool": "mesh_mask_time", "runs": a.runs}
    verts, faces, _ = cases.load_example_obj()
    v, f = mesh_mask.upload_mesh(cases.example_obj_world(verts), faces, dev)
    focal = 0.5 * 800 / math.tan(0.5 * cases.EXAMPLE_CAMERA_ANGLE_X)
    res["example_obj_800"] = time_case("example OBJ", v, f, cases.EXAMPLE_C2W, 800, 800, focal, a.runs)
    G = a.ball
    ax = torch.arange(G, device=dev, dtype=torch.float32) - (G - 1) * 0.5
    field = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) < (0.3 * G) ** 2
    bv, bf = marching_cubes.marching_cubes(field, 0.5)
    del field
    bv = (bv / (G - 1) - 0.5) * 3.0                                   # into [-1.5, 1.5]^3, the example scene's box
    res[f"ball_{G}_1080p"] = time_case(f"ball {G}^3", bv.contiguous(), bf, cases.EXAMPLE_C2W, 1080, 1920, 0.5 * 1920 / math.tan(0.5 * 0.9), a.runs)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
