"""Profiling helper (not part of the product): time the scene loader (rnerf_images_prepare, datasets.get_dataset).

    python tools/scene_load_time.py [--runs 20] [--views 100] [--size 800] [--loads 3] [--out f.json]

Two cases at the synthetic configs' setting, --views views of --size x --size RGBA at `factor: 2`: (a) rnerf_images_prepare alone on
views that are already on the device as uint8, into a preallocated tensor — HIP events around each call, two warm-up runs, the median
of --runs, and the bytes it reads and writes over that time (input + output exceed the 256 MB last-level cache at the default size);
(b) the whole load of a Blender scene written to a temporary directory (smooth pictures with a little noise, PNG level 6): wall time of
datasets.get_dataset("test", ...) up to a device synchronisation, best and median of --loads, beside the wall time of decoding the same
files alone (datasets.decode_views, the same pool of 8 threads) — the share of the load that is PNG decoding on the host.  One JSON
line at the end."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import datasets, ops, utils      # noqa: E402


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


def write_scene(directory, views, size, rng):
    from PIL import Image
    os.makedirs(os.path.join(directory, "test"))
    yy, xx = np.meshgrid(np.linspace(-1, 1, size), np.linspace(-1, 1, size), indexing="ij")
    noise = rng.normal(0, 2, (size, size, 4))

    def one(i):
        ph = 2 * np.pi * i / views
        rgb = np.stack([0.5 + 0.5 * np.sin(5 * xx + ph), 0.5 + 0.5 * np.cos(4 * yy - ph), 0.5 + 0.5 * np.sin(3 * (xx + yy) + ph)], -1)
        alpha = np.clip(8 * (0.8 - np.hypot(xx, yy)), 0, 1)[..., None]
        im = np.concatenate([rgb, alpha], -1) * 255 + np.roll(noise, 7 * i, axis=1)
        Image.fromarray(np.clip(im, 0, 255).astype(np.uint8)).save(os.path.join(directory, "test", f"r_{i}.png"), "PNG")
        return {"file_path": f"./test/r_{i}", "transform_matrix": np.eye(4).tolist()}

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as pool:
        frames = list(pool.map(one, range(views)))
    with open(os.path.join(directory, "transforms_test.json"), "w") as fp:
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, fp)
    return sum(os.path.getsize(os.path.join(directory, "test", f)) for f in os.listdir(os.path.join(directory, "test")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--loads", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the device: it needs one"
    dev = torch.device("cuda:0")
    n, s = a.views, a.size
    u8 = torch.randint(0, 256, (n, s, s, 4), dtype=torch.uint8, device=dev)
    out = torch.empty((n, s // 2, s // 2, 3), dtype=torch.float32, device=dev)
    moved = u8.numel() + out.numel() * 4
    res = {"tool": "scene_load_time", "runs": a.runs, "views": n, "height": s, "width": s, "channels": 4, "factor": 2, "bytes_moved": moved}
    for name, white in (("prepare_ms", False), ("prepare_white_ms", True)):
        res[name] = median_ms(lambda: ops.images_prepare(u8, 2, white, out=out), a.runs)
    res["prepare_gb_per_s"] = moved / res["prepare_ms"]["median"] / 1e6
    del u8, out
    with tempfile.TemporaryDirectory() as d:
        res["png_bytes"] = write_scene(d, n, s, np.random.default_rng(0))
        flags = utils.default_flags(dataset="blender", data_dir=d, factor=2, white_bkgd=False)
        files = datasets.blender_index("test", flags).files
        loads, decodes = [], []
        for _ in range(a.loads):
            t0 = time.perf_counter()
            datasets.decode_views(files)
            decodes.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = datasets.get_dataset("test", flags, device=dev)
            torch.cuda.synchronize()
            loads.append(time.perf_counter() - t0)
            assert tuple(ds.images.shape) == (n, s // 2, s // 2, 3)
            del ds
    res.update(load_s={"median": float(np.median(loads)), "min": min(loads)}, decode_only_s={"median": float(np.median(decodes)), "min": min(decodes)},
               decode_workers=datasets.DECODE_WORKERS)
    print(f"{n} views of {s} x {s} x 4 at factor 2: rnerf_images_prepare median {res['prepare_ms']['median']:.3f} ms ({res['prepare_gb_per_s']:.0f} GB/s over "
          f"{moved / 1e6:.0f} MB), with the white composite {res['prepare_white_ms']['median']:.3f} ms; whole load median {res['load_s']['median']:.2f} s, "
          f"decoding alone {res['decode_only_s']['median']:.2f} s ({datasets.DECODE_WORKERS} threads, {res['png_bytes'] / 1e6:.0f} MB of PNG)")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
