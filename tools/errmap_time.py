"""Profiling helper (not part of the product): time what evaluate(errmap=True) adds per view (errmap.error_maps, errmap.sheet).

    python tools/errmap_time.py [--runs 20] [--size 800] [--out f.json]

On a smooth --size x --size image pair already on the device: (a) errmap.quantize8 of the prediction; (b) errmap.error_maps — the
squared-error map and mean (2 launches), the summary SSIM (3: tiles, channel mean, mean), FLIP (3) and the three torch launches of the
PSNR value; (c) errmap.sheet, one launch; (d) the read-back of the sheet, the one transfer a view with save_output adds.  HIP events
around each call, the workspace allocations of the host layer included.  Two warm-up runs, then the median of --runs.  One JSON line at
the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenerfro_amd import errmap      # noqa: E402


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
    ref = np.stack([0.5 + 0.4 * np.sin(3 * xx + c) * np.cos(2 * yy - c) for c in range(3)], -1)
    reference = torch.from_numpy(ref.astype(np.float32)).to(dev)
    pred = torch.from_numpy((ref + 0.03 * rng.standard_normal(ref.shape)).astype(np.float32)).to(dev)
    test = errmap.quantize8(pred)
    maps = errmap.error_maps(reference, test)
    three = [maps[k] for k in errmap.MAP_NAMES]
    sheet = errmap.sheet(reference, test, three)
    res = {"tool": "errmap_time", "runs": a.runs, "height": n, "width": n, "sheet_bytes": int(sheet.numel()),
           "quantize8_ms": median_ms(lambda: errmap.quantize8(pred), a.runs),
           "error_maps_ms": median_ms(lambda: errmap.error_maps(reference, test), a.runs),
           "sheet_ms": median_ms(lambda: errmap.sheet(reference, test, three), a.runs),
           "sheet_readback_ms": median_ms(lambda: sheet.cpu(), a.runs)}
    res["per_view_ms"] = res["quantize8_ms"]["median"] + res["error_maps_ms"]["median"] + res["sheet_ms"]["median"]
    print(f"{n} x {n}: quantize8 {res['quantize8_ms']['median']:.3f} ms, error_maps {res['error_maps_ms']['median']:.3f} ms, sheet "
          f"{res['sheet_ms']['median']:.3f} ms ({res['sheet_bytes']} bytes; read-back {res['sheet_readback_ms']['median']:.3f} ms): "
          f"{res['per_view_ms']:.3f} ms per view on the device")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
