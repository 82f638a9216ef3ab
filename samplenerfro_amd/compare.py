"""A/B comparison of two runs on the device: metric/compare.py (which run has the lower error, per pixel and metric) and metric/export.py's
export_video (the runs and the ground truth side by side), over rnerf_compare_sheet and rnerf_compare_strip (csrc/errmap.hip) and the
maps of errmap.error_maps — without imageio, cv2 or a float map crossing the bus.

metric_maps(reference, test) gives the four maps compare.py compares (squared error, 1 - SSIM, LPIPS with weights, LDR-FLIP);
win_loss(maps_a, maps_b, H, W) is `compare_{METHOD2}/frame/frame_NNN.png` as bytes on the device, with the number of pixels each run
wins per metric, and the `{psnr,dssim,lpips,flip}_NNN.png` are slices of it (panels, write_frames); strip(images, reference, rect) is one
frame of export_video; compare_views runs the loop of compare.py:166-239 over two sets of predictions.  Every function but
compare_views returns device tensors and synchronises nothing; numpy arrays and CPU tensors are uploaded to the device of the other
arguments, or to the current device.  There is no CPU fallback.

Deviations from the reference, all three in what is drawn or read, none in a number:
  - the cv2 text labels (put_text, compare.py:232, export.py:111-115) are not drawn;
  - the mp4 (compare.py:242, export.py:135) is not written: the frames are, as PNGs;
  - compare.py:180's `- 1` on the OpenCV centre crop is not reproduced — it makes the ground truth one pixel smaller than the
    predictions (torch.mean((ref - src)**2) then fails to broadcast), so that branch cannot have run; the views are taken as the dataset
    yields them."""
from __future__ import annotations

import glob
import os
from typing import Iterable, Optional

import numpy as np
import torch

from . import errmap, ops, utils

GAP = errmap.GAP                          # compare.py:234, export.py:128: columns of 255 between the panels
MAP_NAMES = ("psnr", "dssim", "flip")     # compare.py:218 without "lpips"
MAP_NAMES_LPIPS = ("psnr", "dssim", "lpips", "flip")      # compare.py:218
CLASSES = ("a", "tie", "b", "neither")    # the columns of the counts


def metric_maps(reference, test, lpips=None, pixels_per_degree=utils.FLIP_PPD_SUMMARY) -> dict:
    """The maps and numbers of compare.py:203-213 for one run and one view: errmap.error_maps' dictionary ("psnr", "ssim", "flip", with
    lpips "lpips", and their "_value"s) plus "dssim": [H-10, W-10], 1 - clip(ssim, 0, 1) in float32 (:97-102), and "dssim_value":
    1 - ssim_value."""
    res = errmap.error_maps(reference, test, pixels_per_degree=pixels_per_degree, lpips=lpips)
    res["dssim"] = 1.0 - res["ssim"].clamp(0.0, 1.0)
    res["dssim_value"] = 1.0 - res["ssim_value"]
    return res


def win_loss(maps_a, maps_b, H: int, W: int, counts: bool = True):
    """compare.py:216-236 -> (frame uint8 [H, K (W + 5), 3] on the device, counts int64 [K, 4] or None).  maps_a, maps_b: the K <= 4
    error maps of run A and of run B ([h_k, w_k], h_k <= H, w_k <= W).  A pixel is orange (239, 138, 98) where A's error is lower or
    equal, blue (103, 169, 207) where B's is lower, near-white (247, 247, 247) where they are within 1e-3, black where either is NaN;
    each map lies in the top-left corner of a white H x W panel, 5 white columns after every panel.  counts[k] = the pixels of map k
    that are {A's, tied, B's, neither's} (CLASSES)."""
    dev = ops.device_of(*maps_a, *maps_b)
    return ops.compare_sheet([ops.as_f32(m, dev) for m in maps_a], [ops.as_f32(m, dev) for m in maps_b], H, W, counts=counts)


def panels(frame, shapes):
    """The coloured maps inside a frame: shapes = [(h_k, w_k), ...] in the frame's order -> a list of views [h_k, w_k, 3]."""
    K = len(shapes)
    width = int(frame.shape[1])
    if K < 1 or width % K:
        raise ValueError(f"panels: a frame {width} columns wide does not hold {K} panels")
    W = width // K - GAP
    return [frame[:int(h), k * (W + GAP):k * (W + GAP) + int(w)] for k, (h, w) in enumerate(shapes)]


def _as_u8(img, dev: torch.device) -> torch.Tensor:
    """uint8 [H, W, 3] on dev.  uint8 stays; floats go through utils.save_img's conversion, trunc(clip(x, 0, 1) * 255) in float32 (NaN
    gives 0)."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    t = t.to(dev)
    if t.dtype != torch.uint8:
        t = torch.nan_to_num(t.to(torch.float32), nan=0.0).clamp(0.0, 1.0).mul(255.0).to(torch.uint8)
    return t[..., :3].contiguous()


def strip(images, reference, rect=None) -> torch.Tensor:
    """One frame of export.py:92-133 -> uint8 [H, N (W + 5) + W, 3] on the device: the N <= 4 images, 5 white columns after each, then
    the reference.  images, reference: [H, W, 3], uint8 or float (floats become the bytes utils.save_img writes).  rect: None or
    (x, y, w, h) as mesh_mask.bounding_rect gives it — the images, not the reference, are faded half-way to white outside it
    (:102-108)."""
    images = list(images)
    dev = ops.device_of(reference, *images)
    return ops.compare_strip([_as_u8(im, dev) for im in images], _as_u8(reference, dev), rect)


def load_preds(directory: str):
    """The `???.png` of a run's test_preds directory in sorted order (compare.py:69), each a uint8 array [H, W, 3] through PIL."""
    from PIL import Image
    for path in sorted(glob.glob(os.path.join(directory, "???.png"))):
        yield np.asarray(Image.open(path))[..., :3]


def compare_dir(out_dir: str, name_b: str = "b", suffix: str = "") -> str:
    """compare.py:154: compare_{METHOD2}{suffix} under out_dir."""
    return os.path.join(out_dir, f"compare_{name_b}{suffix}")


def write_frames(out_dir: str, idx: int, frame, shapes, name_b: str = "b", suffix: str = "", strip_image=None) -> None:
    """compare.py:154-157,228,236: compare_{name_b}{suffix}/psnr_{idx:03d}.png, dssim_..., flip_... (the frame's panels; with four
    shapes also lpips_...) and compare_{name_b}{suffix}/frame{suffix}/frame_{idx:03d}.png (the frame) under out_dir, through PIL; with
    strip_image also compare_{name_b}{suffix}/strip{suffix}/strip_{idx:03d}.png.  frame, strip_image: device tensors (read back here,
    once each) or arrays."""
    from PIL import Image
    if len(shapes) not in (len(MAP_NAMES), len(MAP_NAMES_LPIPS)):
        raise ValueError(f"write_frames: need the shapes of the {MAP_NAMES} or {MAP_NAMES_LPIPS} maps, got {len(shapes)}")
    names = MAP_NAMES_LPIPS if len(shapes) == len(MAP_NAMES_LPIPS) else MAP_NAMES
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    frame = host(frame)
    cmp_dir = compare_dir(out_dir, name_b, suffix)
    frame_dir = os.path.join(cmp_dir, "frame" + suffix)
    os.makedirs(frame_dir, exist_ok=True)
    for name, panel in zip(names, panels(frame, shapes)):
        Image.fromarray(np.ascontiguousarray(panel)).save(os.path.join(cmp_dir, f"{name}_{idx:03d}.png"), "PNG")
    Image.fromarray(np.ascontiguousarray(frame)).save(os.path.join(frame_dir, f"frame_{idx:03d}.png"), "PNG")
    if strip_image is not None:
        strip_dir = os.path.join(cmp_dir, "strip" + suffix)
        os.makedirs(strip_dir, exist_ok=True)
        Image.fromarray(np.ascontiguousarray(host(strip_image))).save(os.path.join(strip_dir, f"strip_{idx:03d}.png"), "PNG")


_u8_tables: dict = {}                     # device -> float32 [256]: i / 255 rounded once, as numpy divides


def _pred_f32(pred, dev: torch.device) -> torch.Tensor:
    """A prediction as compare.py's load_img reads its PNG (:36): uint8 / 255 in float32 (through a table made by numpy, so that the
    quotient is the correctly rounded one); a float render through errmap.quantize8, which gives the same values."""
    if (pred.dtype == torch.uint8) if isinstance(pred, torch.Tensor) else (np.asarray(pred).dtype == np.uint8):
        table = _u8_tables.get(dev)
        if table is None:
            table = _u8_tables[dev] = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(dev)
        return table[_as_u8(pred, dev).to(torch.int64)]
    return errmap.quantize8(ops.as_f32(pred, dev)[..., :3].contiguous())


def compare_views(views: Iterable[dict], preds_a: Iterable, preds_b: Iterable, *, masks=None, mask_mode: Optional[str] = None, lpips=None,
                  pixels_per_degree=utils.FLIP_PPD_SUMMARY, out_dir: Optional[str] = None, name_b: str = "b", save_output: bool = False,
                  strips: bool = False, keep_frames: bool = False) -> dict:
    """The loop of compare.py:166-239 over two runs' predictions of the same views.

    views: batches as datasets.get_dataset("test", ...) or evaluate.device_views yield them ("pixels": [H, W, 3]); preds_a, preds_b:
    iterables of [H, W, 3] images, one per view — uint8 is taken as read from a PNG (load_preds), a float render goes through
    errmap.quantize8, so two live models compare exactly as their PNGs would (a generator over utils.render_image serves).

    masks + mask_mode: exactly evaluate.apply_mask ("mask": ground truth and both predictions are multiplied by the mask; "crop": all
    three are cut to its bounding rectangle; "mask_crop": both, compare.py:187-197); the directory names carry evaluate.mask_suffix —
    compare.py:153 has the precedence quirk of summary.py:165, "_mask" for "mask" and "mask_crop", "_crop" for "crop".

    Per view: two metric_maps, one win_loss, with strips one strip (the uncropped images; in the crop modes the rectangle is the mask's
    mesh_mask.bounding_rect, export.py:92-108), and one read-back of the 2 K values and 4 K counts.  With save_output, write_frames
    writes out_dir/compare_{name_b}{suffix}/{psnr,dssim,lpips,flip}_{idx:03d}.png, .../frame{suffix}/frame_{idx:03d}.png and, with
    strips, .../strip{suffix}/strip_{idx:03d}.png (one uint8 image read back for each).  lpips: a weights object (lpips.load_weights)
    adds the LPIPS map as the third of four (MAP_NAMES_LPIPS).

    -> {"names": the K metric names, "a", "b": {name: per-view values} (PSNR in dB — the higher the better, the only one; 1 - SSIM, LPIPS,
    FLIP), "counts": per view a K x 4 list of ints {A wins, tie, B wins, neither} (CLASSES), "shares": {name: {"a", "tie", "b",
    "neither"}} the shares of all compared pixels over all views, "mean_a", "mean_b": {name: mean over the views}, "shapes": per view
    the K map shapes}; with keep_frames also "frames" (and "strips"): the device tensors of every view.  Too few or too many
    predictions or masks, an image whose shape is not the view's, a (cropped) view below the 11 x 11 SSIM window, or below 31 x 31
    with lpips, is a ValueError naming the view.  The labels, the mp4 and compare.py:180's `- 1` are left out (see the module's text)."""
    from . import evaluate, mesh_mask
    if (masks is None) != (mask_mode is None):
        raise ValueError("compare_views: masks and mask_mode go together (got only one of them)")
    suffix = evaluate.mask_suffix(mask_mode)
    if save_output and out_dir is None:
        raise ValueError("compare_views: save_output needs out_dir")
    names = MAP_NAMES_LPIPS if lpips is not None else MAP_NAMES
    K = len(names)
    iters = {"preds_a": iter(preds_a), "preds_b": iter(preds_b)}
    if masks is not None:
        iters["masks"] = iter(masks)
    res = {"names": names, "a": {n: [] for n in names}, "b": {n: [] for n in names}, "counts": [], "shapes": []}
    if keep_frames:
        res["frames"] = []
        if strips:
            res["strips"] = []
    idx = -1
    for idx, batch in enumerate(views):
        got = {}
        for what, it in iters.items():
            try:
                got[what] = next(it)
            except StopIteration:
                raise ValueError(f"compare_views: {what} ran out at view {idx}") from None
        pixels = batch["pixels"]
        dev = ops.device_of(pixels, got["preds_a"], got["preds_b"])
        pixels = ops.as_f32(pixels, dev)[..., :3].contiguous()
        for what in ("preds_a", "preds_b"):
            if tuple(np.shape(got[what]))[:2] != tuple(pixels.shape[:2]) or len(np.shape(got[what])) != 3:
                raise ValueError(f"compare_views: view {idx} is {tuple(pixels.shape)}, its image of {what} {tuple(np.shape(got[what]))}")
        a, b = _pred_f32(got["preds_a"], dev), _pred_f32(got["preds_b"], dev)
        rect = None
        if strips:
            full = (got["preds_a"], got["preds_b"], pixels)           # the bytes of the PNGs, unmasked and uncropped
        if mask_mode is not None:
            try:
                both, ref = evaluate.apply_mask(torch.cat([a, b], dim=-1), pixels, got["masks"], mask_mode)
            except ValueError as e:
                raise ValueError(f"compare_views: view {idx}: {e}") from None
            a, b = both[..., :3].contiguous(), both[..., 3:].contiguous()
            if strips and mask_mode in ("crop", "mask_crop"):
                rect = mesh_mask.bounding_rect(got["masks"])
        else:
            ref = pixels
        H, W = int(ref.shape[0]), int(ref.shape[1])
        if H < 11 or W < 11:
            raise ValueError(f"compare_views: view {idx} is compared at {H} x {W} pixels, smaller than the 11 x 11 SSIM window")
        if lpips is not None and (H < ops.LPIPS_MIN_SIZE or W < ops.LPIPS_MIN_SIZE):
            raise ValueError(f"compare_views: view {idx} is compared at {H} x {W} pixels, LPIPS needs at least {ops.LPIPS_MIN_SIZE} x "
                             f"{ops.LPIPS_MIN_SIZE}")
        ma = metric_maps(ref, a, lpips=lpips, pixels_per_degree=pixels_per_degree)
        mb = metric_maps(ref, b, lpips=lpips, pixels_per_degree=pixels_per_degree)
        frame, counts = win_loss([ma[n] for n in names], [mb[n] for n in names], H, W)
        strip_image = strip(full[:2], full[2], rect) if strips else None
        values = torch.stack([m[n + "_value"] for m in (ma, mb) for n in names]).to(torch.float64)
        back = torch.cat([values, counts.reshape(-1).to(torch.float64)]).cpu()            # the one read-back of the view: 6 K doubles
        for k, n in enumerate(names):
            res["a"][n].append(float(back[k]))
            res["b"][n].append(float(back[K + k]))
        res["counts"].append([[int(v) for v in back[2 * K + 4 * k:2 * K + 4 * k + 4]] for k in range(K)])
        shapes = [tuple(ma[n].shape) for n in names]
        res["shapes"].append(shapes)
        if keep_frames:
            res["frames"].append(frame)
            if strips:
                res["strips"].append(strip_image)
        if save_output:
            write_frames(out_dir, idx, frame, shapes, name_b, suffix, strip_image)
    for what, it in iters.items():
        if next(it, None) is not None:
            raise ValueError(f"compare_views: {what} holds more than the {idx + 1} views (view {idx + 1} has no ground truth)")
    total = np.asarray(res["counts"], np.int64).reshape(-1, K, 4).sum(0)
    res["shares"] = {n: {c: (float(total[k, j]) / float(total[k].sum()) if total[k].sum() else None) for j, c in enumerate(CLASSES)}
                     for k, n in enumerate(names)}
    mean = lambda v: float(np.mean(np.array(v))) if v else None
    res["mean_a"] = {n: mean(res["a"][n]) for n in names}
    res["mean_b"] = {n: mean(res["b"][n]) for n in names}
    if mask_mode is not None:
        res["mask_mode"] = mask_mode
    return res
