"""Held-out evaluation: the loop of eval.py:155-215 (and the validation block of train.py:429-456) without the JAX plumbing.

`device_views` yields the batches eval.py reads ({"rays", "pixels"}) with the rays generated on the device; `evaluate` renders each view
with utils.render_image (pipelined form), scores it on the device — PSNR of the device MSE (utils.compute_psnr) and SSIM with max_val 1
(utils.compute_ssim, rnerf_ssim) — and reads back two floats per view.  With save_output it writes the reference's files.  With flip=True
each view is also scored with LDR-FLIP (utils.compute_flip, rnerf_flip; metric/summary.py:72-78) and the read-back carries three floats.
"""
from __future__ import annotations

import os
import time
from typing import Iterable, Optional

import numpy as np
import torch

from . import ops, utils
from .utils import Rays


def device_views(images, camtoworlds, *, focal: Optional[float] = None, cam_mat=None, pixel_center: bool = True, device):
    """One {"rays": Rays([H, W, 3] origins, None, [H, W, 3] viewdirs, None), "pixels": [H, W, 3]} per view, on `device`.

    images: [n, H, W, >=3] (numpy array, tensor, or a sequence of per-view images); camtoworlds: [n, 3 or 4, 4].  The rays are
    ops.generate_rays (bit-equal to Dataset._generate_rays, rnerf/datasets.py:216-242 with `focal`, :486-518 with `cam_mat`)."""
    for img, c2w in zip(images, camtoworlds):
        if isinstance(c2w, torch.Tensor):
            c2w = c2w.detach().cpu().numpy()
        H, W = int(img.shape[0]), int(img.shape[1])
        o, _, v = ops.generate_rays(c2w, H, W, device, focal=focal, cam_mat=cam_mat, pixel_center=pixel_center)
        if isinstance(img, torch.Tensor):
            pix = img[..., :3].to(device=device, dtype=torch.float32).contiguous()
        else:
            pix = torch.from_numpy(np.ascontiguousarray(np.asarray(img)[..., :3], dtype=np.float32)).to(device)
        yield {"rays": Rays(o, None, v, None), "pixels": pix}


def write_metric_files(out_dir: str, step, psnr_values, ssim_values, flip_values=None) -> None:
    """eval.py:207-215: psnrs_{step}.txt / ssims_{step}.txt (the values joined by spaces) and psnr.txt / ssim.txt (their means).  With
    flip_values also flips_{step}.txt / flip.txt in the same style (not files of the reference)."""
    with open(os.path.join(out_dir, f"psnrs_{step}.txt"), "w") as f:
        f.write(" ".join([str(v) for v in psnr_values]))
    with open(os.path.join(out_dir, f"ssims_{step}.txt"), "w") as f:
        f.write(" ".join([str(v) for v in ssim_values]))
    with open(os.path.join(out_dir, "psnr.txt"), "w") as f:
        f.write("{}".format(np.mean(np.array(psnr_values))))
    with open(os.path.join(out_dir, "ssim.txt"), "w") as f:
        f.write("{}".format(np.mean(np.array(ssim_values))))
    if flip_values is not None:
        with open(os.path.join(out_dir, f"flips_{step}.txt"), "w") as f:
            f.write(" ".join([str(v) for v in flip_values]))
        with open(os.path.join(out_dir, "flip.txt"), "w") as f:
            f.write("{}".format(np.mean(np.array(flip_values))))


def evaluate(model, variables, views: Iterable[dict], rng, *, chunk: int = 8192, normalize_disp: bool = False, out_dir: Optional[str] = None,
             step=None, save_output: bool = False, render_path: bool = False, flip: bool = False,
             flip_pixels_per_degree: Optional[float] = None) -> dict:
    """Render and score every view (eval.py:155-215).

    model / variables: what models.construct_nerf returns; views: batches as device_views yields them; rng: the render key (eval.py passes
    the same key for every view).  render_path: the views have no ground truth (no metrics, no metric files).  save_output: write
    {idx:03d}.png and disp_{idx:03d}.png into out_dir, and (unless render_path) the metric files of write_metric_files for `step`.

    -> {"psnrs", "ssims": per-view Python floats, "psnr", "ssim": their means (None without views or with render_path), "seconds": wall
    time of the loop, "rays_per_sec": rendered rays over it (train.py:450-452)}.

    flip=True also scores each view with utils.compute_flip(pred_color, pixels, flip_pixels_per_degree) (None: compute_ldrflip's default;
    utils.FLIP_PPD_SUMMARY is what metric/summary.py uses): the result gains "flips" and "flip", save_output also writes
    flips_{step}.txt and flip.txt.  With flip=False the keys, the files and the launches are those of the loop without it."""
    if save_output:
        if out_dir is None:
            raise ValueError("evaluate: save_output needs out_dir")
        os.makedirs(out_dir, exist_ok=True)

    def render_fn(key_0, key_1, rays, path=None):
        return model.apply(variables, key_0, key_1, rays, False, path=path)

    psnr_values, ssim_values, flip_values = [], [], []
    num_rays = 0
    t0 = time.perf_counter()
    for idx, batch in enumerate(views):
        pred_color, pred_disp, _pred_acc = utils.render_image(render_fn, batch["rays"], rng, normalize_disp, chunk=chunk, model=model)
        num_rays += int(pred_color.shape[0]) * int(pred_color.shape[1])
        if not render_path:
            psnr = utils.compute_psnr(((pred_color - batch["pixels"]) ** 2).mean())
            ssim = utils.compute_ssim(pred_color, batch["pixels"], max_val=1.0)
            scores = [psnr.to(torch.float32), ssim]
            if flip:
                scores.append(utils.compute_flip(pred_color, batch["pixels"], flip_pixels_per_degree))
            pair = torch.stack(scores).cpu()                                  # the one read-back of the view: 8 bytes (12 with flip)
            psnr_values.append(float(pair[0]))
            ssim_values.append(float(pair[1]))
            if flip:
                flip_values.append(float(pair[2]))
        if save_output:
            utils.save_img(pred_color, os.path.join(out_dir, "{:03d}.png".format(idx)))
            utils.save_img(pred_disp[..., 0], os.path.join(out_dir, "disp_{:03d}.png".format(idx)))
    if num_rays:
        torch.cuda.synchronize(pred_color.device)
    seconds = time.perf_counter() - t0
    if save_output and not render_path:
        write_metric_files(out_dir, step, psnr_values, ssim_values, flip_values if flip else None)
    have = bool(psnr_values)
    res = {"psnrs": psnr_values, "ssims": ssim_values,
           "psnr": float(np.mean(np.array(psnr_values))) if have else None,
           "ssim": float(np.mean(np.array(ssim_values))) if have else None,
           "seconds": seconds, "rays_per_sec": num_rays / seconds if seconds > 0 else 0.0}
    if flip:
        res["flips"] = flip_values
        res["flip"] = float(np.mean(np.array(flip_values))) if flip_values else None
    return res
