"""The per-view error maps and the comparison sheet of metric/summary.py on the device (rnerf_errmap_mse, rnerf_ssim_summary, rnerf_flip,
rnerf_lpips, rnerf_errmap_sheet; csrc/errmap.hip, csrc/metrics.hip, csrc/lpips.hip), without imageio, cv2 or a float map crossing the bus.

error_maps(reference, test) gives the three maps summary.py colours (squared error, the pytorch-msssim SSIM, LDR-FLIP) and its three
numbers; sheet(reference, test, maps) is `errmap/frame/frame_NNN.png` as bytes on the device, and the three `errmap/*_NNN.png` are
slices of it (write_error_maps).  evaluate.evaluate(errmap=True) calls them for every view.  The LPIPS map and column come with
lpips=weights (lpips.load_weights: the weights are not part of this repository); without it they are left out and nothing else changes.
NaN in an image or a map gives byte or colour index 0 (the reference's cast is undefined
there).  Every function returns device tensors and synchronises nothing; numpy arrays and CPU tensors are uploaded to the device of the
other argument, or to the current device.  There is no CPU fallback."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops, utils

GAP = 5                                   # summary.py:231,238: columns of ones between the panels
MAP_NAMES = ("psnr", "ssim", "flip")      # summary.py:232 without "lpips"
MAP_NAMES_LPIPS = ("psnr", "ssim", "lpips", "flip")      # summary.py:232


_q8_tables: dict = {}                     # device -> float32 [256]: i / 255 as the reader of a PNG forms it


def quantize8(img):
    """What a reader of utils.save_img's PNG gets back (summary.py:30-38 after rnerf/utils.py:474-488): trunc(clip(x, 0, 1) * 255) / 255 in
    float32, on the device.  summary.py scores the PNG on disk, not the float render.  NaN gives 0."""
    dev = ops.device_of(img)
    x = ops.as_f32(img, dev)
    table = _q8_tables.get(dev)
    if table is None:
        table = _q8_tables[dev] = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(dev)
    idx = torch.nan_to_num(x, nan=0.0).clamp(0.0, 1.0).mul(255.0).to(torch.int64)
    return table[idx]


def error_maps(reference, test, pixels_per_degree=utils.FLIP_PPD_SUMMARY, lpips=None) -> dict:
    """The maps and numbers of summary.py:212-215 for one view.  reference, test: [H, W, 3] (H, W >= 11), numpy or tensors.
    -> {"psnr": [H, W] the squared-error map (:54), "ssim": [H-10, W-10] the channel mean of ssim.py's map, unclipped (:58), "flip":
    [H, W] (:77), "psnr_value": -20 log10(sqrt(mse)) (:51-52), "ssim_value", "flip_value": 0-dim float32}, all on the device.  lpips: a weights object
    (lpips.load_weights) adds "lpips": [H, W], the LPIPS map clipped to [0, 1] (:66-67), and "lpips_value" (:68); H, W >= 31 then."""
    s0, s1 = tuple(np.shape(reference)), tuple(np.shape(test))
    if s0 != s1 or len(s0) != 3 or s0[2] != 3:
        raise ValueError(f"error_maps: need two [H, W, 3] images, got shapes {s0} and {s1}")
    if s0[0] < 11 or s0[1] < 11:
        raise ValueError(f"error_maps: the images ({s0[0]} x {s0[1]}) are smaller than the 11 x 11 SSIM window")
    dev = ops.device_of(reference, test)
    a, b = ops.as_f32(reference, dev), ops.as_f32(test, dev)
    mse_map, mse = ops.errmap_mse(a, b)
    ssim_map, ssim = ops.ssim_summary(a, b, data_range=1.0)
    flip_map, flip = ops.flip(a, b, pixels_per_degree=float(pixels_per_degree), return_both=True)
    res = {"psnr": mse_map, "ssim": ssim_map, "flip": flip_map, "psnr_value": -20.0 * torch.log10(torch.sqrt(mse)), "ssim_value": ssim,
           "flip_value": flip}
    if lpips is not None:
        if s0[0] < ops.LPIPS_MIN_SIZE or s0[1] < ops.LPIPS_MIN_SIZE:
            raise ValueError(f"error_maps: the images ({s0[0]} x {s0[1]}) are smaller than the {ops.LPIPS_MIN_SIZE} x {ops.LPIPS_MIN_SIZE} LPIPS needs")
        lpips_map, lpips_value = ops.lpips(a, b, lpips, return_both=True)
        res["lpips"], res["lpips_value"] = lpips_map.clamp(0.0, 1.0), lpips_value
    return res


def sheet(reference, test, maps) -> torch.Tensor:
    """summary.py:231-240 -> uint8 [H, (2 + K)(W + 5), 3] on the device: reference | test | the K <= 4 maps ([h_k, w_k], h_k <= H,
    w_k <= W) through the magma colours, each in the top-left corner of a black H x W panel; 5 white columns after every panel."""
    dev = ops.device_of(reference, test, *maps)
    return ops.errmap_sheet(ops.as_f32(reference, dev), ops.as_f32(test, dev), [ops.as_f32(m, dev) for m in maps])


def colorize(error_map) -> torch.Tensor:
    """save_err (summary.py:43-45) -> uint8 [h, w, 3] on the device: the panel of a one-map sheet."""
    dev = ops.device_of(error_map)
    m = ops.as_f32(error_map, dev)
    if m.dim() != 2:
        raise ValueError(f"colorize: need a [h, w] map, got shape {tuple(m.shape)}")
    h, w = int(m.shape[0]), int(m.shape[1])
    blank = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    return ops.errmap_sheet(blank, blank, [m])[:, 2 * (w + GAP):2 * (w + GAP) + w].contiguous()


def panels(sheet_image, shapes):
    """The coloured maps inside a sheet: shapes = [(h_k, w_k), ...] in the sheet's order -> a list of views [h_k, w_k, 3]."""
    K = len(shapes)
    width = int(sheet_image.shape[1])
    if width % (2 + K):
        raise ValueError(f"panels: a sheet {width} columns wide does not hold 2 + {K} panels")
    W = width // (2 + K) - GAP
    return [sheet_image[:int(h), (2 + k) * (W + GAP):(2 + k) * (W + GAP) + int(w)] for k, (h, w) in enumerate(shapes)]


def write_error_maps(out_dir: str, idx: int, sheet_image, shapes, suffix: str = "") -> None:
    """summary.py:165-169,223-240: errmap{suffix}/psnr_{idx:03d}.png, ssim_..., flip_... (the sheet's panels) and
    errmap{suffix}/frame{suffix}/frame_{idx:03d}.png (the sheet) under out_dir, through PIL.  sheet_image: uint8 [H, 5 (W + 5), 3], a
    device tensor (read back here, once) or an array; shapes: the (h, w) of the psnr, ssim and flip maps.  Four shapes (psnr, ssim,
    lpips, flip: MAP_NAMES_LPIPS) with a six-panel sheet also write lpips_{idx:03d}.png."""
    from PIL import Image
    if isinstance(sheet_image, torch.Tensor):
        sheet_image = sheet_image.detach().cpu().numpy()
    if len(shapes) not in (len(MAP_NAMES), len(MAP_NAMES_LPIPS)):
        raise ValueError(f"write_error_maps: need the shapes of the {MAP_NAMES} or {MAP_NAMES_LPIPS} maps, got {len(shapes)}")
    names = MAP_NAMES_LPIPS if len(shapes) == len(MAP_NAMES_LPIPS) else MAP_NAMES
    err_dir = os.path.join(out_dir, "errmap" + suffix)
    frame_dir = os.path.join(err_dir, "frame" + suffix)
    os.makedirs(frame_dir, exist_ok=True)
    for name, panel in zip(names, panels(sheet_image, shapes)):
        Image.fromarray(np.ascontiguousarray(panel)).save(os.path.join(err_dir, f"{name}_{idx:03d}.png"), "PNG")
    Image.fromarray(np.ascontiguousarray(sheet_image)).save(os.path.join(frame_dir, f"frame_{idx:03d}.png"), "PNG")


def metric_list_text(psnr_values, ssim_values, flip_values, lpips_values=None) -> str:
    """summary.py:243 per view; without lpips_values, without the LPIPS column (it goes between SSIM and FLIP)."""
    if lpips_values is None:
        return "".join(f"{i:3d}{p:6.2f}{s:6.3f}{f:6.3f}\n" for i, (p, s, f) in enumerate(zip(psnr_values, ssim_values, flip_values)))
    return "".join(f"{i:3d}{p:6.2f}{s:6.3f}{l:6.3f}{f:6.3f}\n"
                   for i, (p, s, l, f) in enumerate(zip(psnr_values, ssim_values, lpips_values, flip_values)))


def result_text(psnr_values, ssim_values, flip_values, lpips_values=None) -> str:
    """summary.py:250; without lpips_values, without the LPIPS column."""
    if lpips_values is None:
        return f"{np.mean(psnr_values):6.2f}{np.mean(ssim_values):6.3f}{np.mean(flip_values):6.3f}\n"
    return f"{np.mean(psnr_values):6.2f}{np.mean(ssim_values):6.3f}{np.mean(lpips_values):6.3f}{np.mean(flip_values):6.3f}\n"


def write_summary_files(out_dir: str, psnr_values, ssim_values, flip_values, suffix: str = "", lpips_values=None) -> None:
    """summary.py:246-250: metric_list{suffix}.txt and result{suffix}.txt."""
    with open(os.path.join(out_dir, f"metric_list{suffix}.txt"), "w") as f:
        f.write(metric_list_text(psnr_values, ssim_values, flip_values, lpips_values))
    with open(os.path.join(out_dir, f"result{suffix}.txt"), "w") as f:
        f.write(result_text(psnr_values, ssim_values, flip_values, lpips_values))
