"""Held-out evaluation: the loop of eval.py:155-215 (and the validation block of train.py:429-456) without the JAX plumbing.

`device_views` yields the batches eval.py reads ({"rays", "pixels"}) with the rays generated on the device; `evaluate` renders each view
with utils.render_image (pipelined form), scores it on the device — PSNR of the device MSE (utils.compute_psnr) and SSIM with max_val 1
(utils.compute_ssim, rnerf_ssim) — and reads back two floats per view.  With save_output it writes the reference's files.  With flip=True
each view is also scored with LDR-FLIP (utils.compute_flip, rnerf_flip; metric/summary.py:72-78) and the read-back carries three floats.
With masks / mask_mode the views are scored on the object's region and / or the crop around it (summary.py:91-92,177-205,
metric/compare.py:132-133,167-197; the masks come from mesh_mask.render_masks).  With vis_suite the depth visualisations of
eval.py:175,196-198 (vis.visualize_suite: rnerf_vis_depth, rnerf_vis_normals) are computed for every view and written with save_output.
With errmap=True every view also gets metric/summary.py's error maps, comparison sheet and numbers (errmap.error_maps, errmap.sheet:
rnerf_errmap_mse, rnerf_ssim_summary, rnerf_flip, rnerf_errmap_sheet), scored on the 8-bit prediction as summary.py scores the PNG.
With lpips=weights (lpips.load_weights) each view is also scored with LPIPS (utils.compute_lpips, rnerf_lpips; summary.py:63-68), and
errmap=True then carries the LPIPS map and column as well.
With path_maps=True every view also gets the refraction maps eval.py:173,195 carries commented out (paths.view_maps: the march again with
its IoR record, reduced per ray by rnerf_path_summary), written with save_output.
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


MASK_MODES = ("mask", "crop", "mask_crop")


def mask_suffix(mask_mode: Optional[str]) -> str:
    """What metric/summary.py:165 evaluates to, `"_mask" if MASK else "" + "_crop" if CROP else ""`.  The conditional expression binds
    more loosely than `+`, so this is "_mask" whenever MASK is set — for "mask" and also for "mask_crop" — and "_crop" for "crop"."""
    if mask_mode is None:
        return ""
    if mask_mode not in MASK_MODES:
        raise ValueError(f"mask_mode must be one of {MASK_MODES} or None, got {mask_mode!r}")
    return "_crop" if mask_mode == "crop" else "_mask"


def write_metric_files(out_dir: str, step, psnr_values, ssim_values, flip_values=None, suffix: str = "", lpips_values=None) -> None:
    """eval.py:207-215: psnrs_{step}.txt / ssims_{step}.txt (the values joined by spaces) and psnr.txt / ssim.txt (their means).  With
    flip_values also flips_{step}.txt / flip.txt in the same style (not files of the reference), with lpips_values lpips_{step}.txt /
    lpips.txt.  suffix (mask_suffix) goes before ".txt" in every name."""
    with open(os.path.join(out_dir, f"psnrs_{step}{suffix}.txt"), "w") as f:
        f.write(" ".join([str(v) for v in psnr_values]))
    with open(os.path.join(out_dir, f"ssims_{step}{suffix}.txt"), "w") as f:
        f.write(" ".join([str(v) for v in ssim_values]))
    with open(os.path.join(out_dir, f"psnr{suffix}.txt"), "w") as f:
        f.write("{}".format(np.mean(np.array(psnr_values))))
    with open(os.path.join(out_dir, f"ssim{suffix}.txt"), "w") as f:
        f.write("{}".format(np.mean(np.array(ssim_values))))
    if flip_values is not None:
        with open(os.path.join(out_dir, f"flips_{step}{suffix}.txt"), "w") as f:
            f.write(" ".join([str(v) for v in flip_values]))
        with open(os.path.join(out_dir, f"flip{suffix}.txt"), "w") as f:
            f.write("{}".format(np.mean(np.array(flip_values))))
    if lpips_values is not None:
        with open(os.path.join(out_dir, f"lpips_{step}{suffix}.txt"), "w") as f:
            f.write(" ".join([str(v) for v in lpips_values]))
        with open(os.path.join(out_dir, f"lpips{suffix}.txt"), "w") as f:
            f.write("{}".format(np.mean(np.array(lpips_values))))


def apply_mask(pred_color: torch.Tensor, pixels: torch.Tensor, mask, mask_mode: str, min_size: int = 11):
    """summary.py:197-205 for one view: -> (pred_color, pixels) multiplied by the mask ("mask", "mask_crop") and then cut to the mask's
    bounding rectangle ("crop", "mask_crop").  mask: [H, W] (or [H, W, 1]), > 0 = set.  min_size: the SSIM window."""
    from . import mesh_mask
    H, W = int(pred_color.shape[0]), int(pred_color.shape[1])
    m = mesh_mask._as_mask(mask, pred_color.device)
    if tuple(m.shape) != (H, W):
        raise ValueError(f"evaluate: a mask of shape {tuple(m.shape)} for a view of {H} x {W}")
    if mask_mode in ("mask", "mask_crop"):
        mf = m.to(torch.float32)[..., None]
        pred_color, pixels = pred_color * mf, pixels * mf
    if mask_mode in ("crop", "mask_crop"):
        x, y, w, h = mesh_mask.bounding_rect(m)
        if w < min_size or h < min_size:
            raise ValueError(f"evaluate: the mask's bounding rectangle is {w} x {h} pixels (an empty mask gives 0 x 0), smaller than the "
                             f"{min_size} x {min_size} SSIM window")
        pred_color, pixels = pred_color[y:y + h, x:x + w].contiguous(), pixels[y:y + h, x:x + w].contiguous()
    return pred_color, pixels


def evaluate(model, variables, views: Iterable[dict], rng, *, chunk: int = 8192, normalize_disp: bool = False, out_dir: Optional[str] = None,
             step=None, save_output: bool = False, render_path: bool = False, flip: bool = False,
             flip_pixels_per_degree: Optional[float] = None, masks=None, mask_mode: Optional[str] = None, vis_suite: bool = False,
             errmap: bool = False, lpips=None, path_maps: bool = False) -> dict:
    """Render and score every view (eval.py:155-215).

    model / variables: what models.construct_nerf returns; views: batches as device_views yields them; rng: the render key (eval.py passes
    the same key for every view).  render_path: the views have no ground truth (no metrics, no metric files).  save_output: write
    {idx:03d}.png and disp_{idx:03d}.png into out_dir, and (unless render_path) the metric files of write_metric_files for `step`.

    -> {"psnrs", "ssims": per-view Python floats, "psnr", "ssim": their means (None without views or with render_path), "seconds": wall
    time of the loop, "rays_per_sec": rendered rays over it (train.py:450-452)}.

    flip=True also scores each view with utils.compute_flip(pred_color, pixels, flip_pixels_per_degree) (None: compute_ldrflip's default;
    utils.FLIP_PPD_SUMMARY is what metric/summary.py uses): the result gains "flips" and "flip", save_output also writes
    flips_{step}.txt and flip.txt.  With flip=False the keys, the files and the launches are those of the loop without it.

    masks + mask_mode: the reference's masked / cropped scores (metric/summary.py MASK / CROP).  masks: one [H, W] mask per view (a
    sequence or iterable of tensors or arrays, e.g. mesh_mask.render_masks; > 0 = set, so 0 / 255 and 0 / 1 both do); mask_mode "mask":
    pred_color and pixels are multiplied by the mask before scoring (summary.py:197-199); "crop": both are cut to the mask's bounding
    rectangle (:201-205); "mask_crop": both, in that order.  The metrics are the same device kernels on those images; PSNR is the mean
    over every pixel of the (cropped) image as there, not normalised by the mask's area.  The metric files carry mask_suffix(mask_mode)
    before ".txt" — "_mask" for "mask" AND for "mask_crop", "_crop" for "crop": summary.py:165's `"_mask" if MASK else "" + "_crop" if
    CROP else ""` parses that way.  The PNGs are written unmasked.  The result gains "mask_mode".  A crop smaller than the SSIM window
    is a ValueError, and so is masks without mask_mode or the reverse; with neither, nothing changes.

    vis_suite=True computes vis.visualize_suite(pred_disp[..., 0], pred_acc[..., 0]) for every view (eval.py:175; seven more launches, no
    read-back); with save_output it also writes depth_{idx:03d}.png, depth_mod_{idx:03d}.png and depth_normals_{idx:03d}.png
    (eval.py:196-198) through utils.save_img.  With vis_suite=False the keys, the files and the launches are those of the loop without it.

    errmap=True: metric/summary.py for every view with ground truth — errmap.error_maps(pixels, errmap.quantize8(pred_color)) (summary.py
    scores the PNG it reads back, not the float render; masked and / or cropped first with masks / mask_mode, :197-205, so a cropped view
    gives a cropped sheet) and one errmap.sheet.  The result gains "summary": {"psnrs", "ssims", "flips", "psnr", "ssim", "flip"}
    (summary.py's PSNR of the quantised image, the pytorch-msssim SSIM, FLIP at utils.FLIP_PPD_SUMMARY); the three floats ride in the
    view's one read-back.  With save_output the sheet is read back (one uint8 image per view) and errmap.write_error_maps writes
    errmap{suffix}/psnr_{idx:03d}.png, ssim_..., flip_... and errmap{suffix}/frame{suffix}/frame_{idx:03d}.png; after the loop
    metric_list{suffix}.txt and result{suffix}.txt (summary.py:243-250 without the LPIPS column).  Not with render_path (ValueError).
    With errmap=False the keys, the files and the launches are those of the loop without it.

    lpips: a weights object (lpips.load_weights / lpips.from_tensors) also scores each view with utils.compute_lpips(pixels, pred_color,
    lpips) on the same (masked and / or cropped) images: the result gains "lpips_values" and "lpips", save_output also writes
    lpips_{step}{suffix}.txt and lpips{suffix}.txt; the float rides in the view's one read-back.  With errmap=True LPIPS is also scored
    on the 8-bit prediction like the rest of the summary: "summary" gains "lpips_values" and "lpips", the clipped map (summary.py:67)
    enters the sheet as the third of four maps (errmap.MAP_NAMES_LPIPS; the sheet is (2 + 4)(W + 5) wide), write_error_maps also writes
    lpips_{idx:03d}.png, and metric_list / result carry the LPIPS column.  A view or crop below 31 x 31 is a ValueError.  With
    lpips=None the keys, the files and the launches are those of the loop without it.

    path_maps=True: paths.view_maps for every view (the view is marched once more, `chunk` rays at a time, with the IoR record; no MLP):
    the result gains "refracted", per view the fraction of rays with a node where |grad n| > 1e-3 (eval.py:173's pred_mask), from an
    integer count read back once per view.  With save_output it also writes mask_{idx:03d}.png (the name at eval.py:195),
    bend_{idx:03d}.png and optical_{idx:03d}.png (paths.visualize_maps through utils.save_img).  Works with render_path as well.  With
    path_maps=False the keys, the files and the launches are those of the loop without it."""
    if errmap and render_path:
        raise ValueError("evaluate: errmap needs ground truth, render_path has none")
    if errmap:
        from . import errmap as em
    if (masks is None) != (mask_mode is None):
        raise ValueError("evaluate: masks and mask_mode go together (got only one of them)")
    suffix = mask_suffix(mask_mode)
    mask_iter = iter(masks) if masks is not None else None
    if save_output:
        if out_dir is None:
            raise ValueError("evaluate: save_output needs out_dir")
        os.makedirs(out_dir, exist_ok=True)

    def render_fn(key_0, key_1, rays, path=None):
        return model.apply(variables, key_0, key_1, rays, False, path=path)

    psnr_values, ssim_values, flip_values, lpips_values = [], [], [], []
    refracted_values = []
    map_names = ()
    if errmap:
        map_names = em.MAP_NAMES_LPIPS if lpips is not None else em.MAP_NAMES
    summary_values = {name: [] for name in map_names}
    num_rays = 0
    t0 = time.perf_counter()
    for idx, batch in enumerate(views):
        pred_color, pred_disp, _pred_acc = utils.render_image(render_fn, batch["rays"], rng, normalize_disp, chunk=chunk, model=model)
        num_rays += int(pred_color.shape[0]) * int(pred_color.shape[1])
        if not render_path:
            scored, pixels = pred_color, batch["pixels"]
            if errmap:
                scored8 = em.quantize8(scored)
                if mask_iter is not None:
                    scored = torch.cat([scored, scored8], dim=-1)             # masked and cropped together with the float render
            if mask_iter is not None:
                try:
                    mask = next(mask_iter)
                except StopIteration:
                    raise ValueError(f"evaluate: masks ran out at view {idx}") from None
                scored, pixels = apply_mask(scored, pixels, mask, mask_mode)
                if errmap:
                    scored, scored8 = scored[..., :3].contiguous(), scored[..., 3:].contiguous()
            psnr = utils.compute_psnr(((scored - pixels) ** 2).mean())
            ssim = utils.compute_ssim(scored, pixels, max_val=1.0)
            scores = [psnr.to(torch.float32), ssim]
            if flip:
                scores.append(utils.compute_flip(scored, pixels, flip_pixels_per_degree))
            if lpips is not None:
                if int(pixels.shape[0]) < ops.LPIPS_MIN_SIZE or int(pixels.shape[1]) < ops.LPIPS_MIN_SIZE:
                    raise ValueError(f"evaluate: view {idx} is scored at {int(pixels.shape[0])} x {int(pixels.shape[1])} pixels, LPIPS needs at "
                                     f"least {ops.LPIPS_MIN_SIZE} x {ops.LPIPS_MIN_SIZE}")
                scores.append(utils.compute_lpips(pixels, scored, lpips))
            if errmap:
                maps = em.error_maps(pixels, scored8, lpips=lpips)
                sheet = em.sheet(pixels, scored8, [maps[name] for name in map_names])
                scores += [maps[name + "_value"] for name in map_names]
            pair = torch.stack(scores).cpu()                                  # the one read-back of the view: 8 bytes (12 with flip)
            psnr_values.append(float(pair[0]))
            ssim_values.append(float(pair[1]))
            if flip:
                flip_values.append(float(pair[2]))
            if lpips is not None:
                lpips_values.append(float(pair[3 if flip else 2]))
            if errmap:
                for name, v in zip(map_names, pair[-len(map_names):]):
                    summary_values[name].append(float(v))
                if save_output:
                    em.write_error_maps(out_dir, idx, sheet, [tuple(maps[name].shape) for name in map_names], suffix)
        if save_output:
            utils.save_img(pred_color, os.path.join(out_dir, "{:03d}.png".format(idx)))
            utils.save_img(pred_disp[..., 0], os.path.join(out_dir, "disp_{:03d}.png".format(idx)))
        if vis_suite:
            from . import vis
            suite = vis.visualize_suite(pred_disp[..., 0], _pred_acc[..., 0])
            if save_output:
                for name in ("depth", "depth_mod", "depth_normals"):
                    utils.save_img(suite[name], os.path.join(out_dir, "{}_{:03d}.png".format(name, idx)))
        if path_maps:
            from . import paths
            pmaps = paths.view_maps(model, variables, batch["rays"], chunk=chunk)
            refracted_values.append(int(pmaps["refracted"].sum()) / pmaps["refracted"].numel())
            if save_output:
                for name, img in paths.visualize_maps(pmaps).items():
                    utils.save_img(img, os.path.join(out_dir, "{}_{:03d}.png".format(name, idx)))
    if num_rays:
        torch.cuda.synchronize(pred_color.device)
    seconds = time.perf_counter() - t0
    if save_output and not render_path:
        write_metric_files(out_dir, step, psnr_values, ssim_values, flip_values if flip else None, suffix,
                           lpips_values if lpips is not None else None)
        if errmap and summary_values["psnr"]:
            em.write_summary_files(out_dir, summary_values["psnr"], summary_values["ssim"], summary_values["flip"], suffix,
                                   summary_values.get("lpips"))
    have = bool(psnr_values)
    res = {"psnrs": psnr_values, "ssims": ssim_values,
           "psnr": float(np.mean(np.array(psnr_values))) if have else None,
           "ssim": float(np.mean(np.array(ssim_values))) if have else None,
           "seconds": seconds, "rays_per_sec": num_rays / seconds if seconds > 0 else 0.0}
    if flip:
        res["flips"] = flip_values
        res["flip"] = float(np.mean(np.array(flip_values))) if flip_values else None
    if lpips is not None:
        res["lpips_values"] = lpips_values
        res["lpips"] = float(np.mean(np.array(lpips_values))) if lpips_values else None
    if mask_mode is not None:
        res["mask_mode"] = mask_mode
    if path_maps:
        res["refracted"] = refracted_values
    if errmap:
        mean = lambda v: float(np.mean(np.array(v))) if v else None
        res["summary"] = {"psnrs": summary_values["psnr"], "ssims": summary_values["ssim"], "flips": summary_values["flip"],
                          "psnr": mean(summary_values["psnr"]), "ssim": mean(summary_values["ssim"]), "flip": mean(summary_values["flip"])}
        if lpips is not None:
            res["summary"]["lpips_values"] = summary_values["lpips"]
            res["summary"]["lpips"] = mean(summary_values["lpips"])
    return res
