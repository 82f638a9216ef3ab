"""Host-side mirror of the parts of rnerf/utils.py that sit on the boundary of the hot path.

Rays / Stats / namedtuple_map / render_image / compute_psnr / compute_ssim / compute_flip (on the device) / save_img / learning_rate_decay /
default flags.  The rest of the reference's utils.py (absl flags, gin, file-system wrappers) is out of scope.
"""
from __future__ import annotations

import collections
import dataclasses
import math
import types
from typing import Callable, Optional

import numpy as np
import torch

from . import prng

# rnerf/utils.py:67 — only origins and viewdirs are read by the path (rnerf/models.py:235-236)
Rays = collections.namedtuple("Rays", ("origins", "directions", "viewdirs", "radii"))


def namedtuple_map(fn, tup):
    """rnerf/utils.py:70-72."""
    return type(tup)(*map(fn, tup))


@dataclasses.dataclass
class Stats:
    """rnerf/utils.py:47-64."""
    loss: float = 0.0
    psnr: float = 0.0
    loss_c: float = 0.0
    psnr_c: float = 0.0
    weight_l2: float = 0.0
    loss_nrm: float = 0.0
    loss_sp: float = 0.0
    annealing_rate: float = 0.0
    loss_bg: float = 0.0
    loss_bg_c: float = 0.0
    loss_bg_smooth: float = 0.0
    coarse_alpha_target: float = 0.0
    fine_alpha_target: float = 0.0


def default_flags(**overrides) -> types.SimpleNamespace:
    """The hot-path subset of rnerf/utils.py:87-245 (flag defaults), overridable like the YAML layer (:248-257)."""
    f = dict(
        config=None, stage="radiance", near=2.0, far=6.0, net_depth=8, net_width=256, net_depth_condition=1,
        net_width_condition=128, weight_decay_mult=0.0, skip_layer=4, num_rgb_channels=3, num_sigma_channels=1,
        randomized=True, min_deg_point=0, max_deg_point=10, deg_view=4, num_coarse_samples=64, num_fine_samples=128,
        use_viewdirs=True, sh_deg=-1, sh_direnc_deg=-1, noise_std=None, lindisp=False, net_activation="relu",
        rgb_activation="sigmoid", sigma_activation="softplus", legacy_posenc_order=False, white_bkgd=True,
        batch_size=1024, lr_init=5e-4, lr_final=5e-6, lr_delay_steps=2500, lr_delay_mult=0.01, grad_max_norm=0.0,
        grad_max_val=0.0, max_steps=1000000, num_path_samples=8, sparsity_weight=0.0, use_fine_sparsity=False,
        use_online_sparsity=True, normal_loss_weight=0.0, normal_smooth_weight=0.0, beta_weight=0.0, bg_weight=0.0,
        bg_smooth_weight=0.0, bg_patch_size=0, chunk=8192,
        # the scene (datasets.get_dataset); factor 4 makes the Blender loader raise, as in the reference: every shipped config sets it
        dataset="blender", data_dir=None, factor=4, skip_frames=1, eval_train=False, render_path=False, use_pixel_centers=False,
        precrop_iters=0, precrop_frac=0.5, batching="single_image",
        backward_precision="f16x3",      # not a reference flag: arithmetic of the HIP backward (train.backward_mode)
        range_retry="lag",               # not a reference flag: re-run a step whose f16-based arithmetic left its range (train.train_step):
                                         # "lag" = decided two steps later (no per-step host read), True = in place (one read per step), False = never
    )
    f.update(overrides)
    return types.SimpleNamespace(**f)


def compute_psnr(mse):
    """rnerf/utils.py:392-401."""
    if isinstance(mse, torch.Tensor):
        return -10.0 / math.log(10.0) * torch.log(mse)
    return -10.0 / math.log(10.0) * math.log(mse)


def compute_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """rnerf/utils.py:404-471 on the device (ops.ssim -> rnerf_ssim); the reference's signature and defaults.

    img0, img1: torch tensors or numpy arrays of one shape [..., H, W, C]; a numpy (or CPU) argument is uploaded to the device of the
    other argument, or to the current device.  Computed in fp32 (the reference with x64 off).  Returns a device tensor: each image's mean
    SSIM (shape [...], 0-dim for one [H, W, C] image) or, with return_map, the map [..., H-fs+1, W-fs+1, C].  Nothing is synchronised:
    `float(ssim)` reads the value back when it is wanted.  There is no CPU fallback."""
    s0, s1 = tuple(np.shape(img0)), tuple(np.shape(img1))
    if s0 != s1:
        raise ValueError(f"compute_ssim: the images differ in shape: {s0} vs {s1}")
    if len(s0) < 3:
        raise ValueError(f"compute_ssim: need [..., H, W, C] images, got shape {s0}")
    if not 1 <= int(filter_size) <= 31:
        raise ValueError(f"compute_ssim: filter_size must be in [1, 31], got {filter_size}")
    if s0[-3] < filter_size or s0[-2] < filter_size:
        raise ValueError(f"compute_ssim: the images ({s0[-3]} x {s0[-2]}) are smaller than the window (filter_size {filter_size})")
    from . import ops
    dev = ops.device_of(img0, img1)
    return ops.ssim(ops.as_f32(img0, dev), ops.as_f32(img1, dev), max_val=max_val, filter_size=filter_size, filter_sigma=filter_sigma, k1=k1, k2=k2,
                    return_map=return_map)


FLIP_PPD_DEFAULT = (0.7 * 3840 / 0.7) * math.pi / 180      # compute_ldrflip's default (flip_api.py:439): a 0.7 m wide 4K monitor at 0.7 m
FLIP_PPD_SUMMARY = 0.3 * (400 / 0.5) * math.pi / 180        # metric/summary.py:72-75


def compute_flip(reference, test, pixels_per_degree=None, return_map=False):
    """LDR-FLIP, compute_ldrflip (metric/flip/flip_api.py:439-495), on the device (ops.flip -> rnerf_flip).

    reference, test: torch tensors or numpy arrays of one shape [..., H, W, 3] (channels last, sRGB in [0, 1]); a numpy (or CPU) argument
    is uploaded to the device of the other argument, or to the current device.  pixels_per_degree: None is compute_ldrflip's default
    (FLIP_PPD_DEFAULT); metric/summary.py scores with FLIP_PPD_SUMMARY.  Computed in fp32.  Returns a device tensor: each image's mean
    error (shape [...], 0-dim for one image: summary.py:78) or, with return_map, the error map [..., H, W].  Nothing is synchronised.
    There is no CPU fallback."""
    s0, s1 = tuple(np.shape(reference)), tuple(np.shape(test))
    if s0 != s1:
        raise ValueError(f"compute_flip: the images differ in shape: {s0} vs {s1}")
    if len(s0) < 3 or s0[-1] != 3:
        raise ValueError(f"compute_flip: need [..., H, W, 3] images, got shape {s0}")
    ppd = FLIP_PPD_DEFAULT if pixels_per_degree is None else float(pixels_per_degree)
    if not (ppd > 0.0 and math.isfinite(ppd)):
        raise ValueError(f"compute_flip: pixels_per_degree must be finite and > 0, got {pixels_per_degree}")
    from . import ops
    dev = ops.device_of(reference, test)
    return ops.flip(ops.as_f32(reference, dev), ops.as_f32(test, dev), pixels_per_degree=ppd, return_map=return_map)


def compute_lpips(img0, img1, weights, return_map=False):
    """LPIPS, lpips.LPIPS(net='alex') v0.1 with normalize=True (metric/summary.py:63-68), on the device (ops.lpips -> rnerf_lpips).

    img0, img1: torch tensors or numpy arrays of one shape [H, W, 3] or [n, H, W, 3] (channels last, in [0, 1], H, W >= 31); a numpy (or
    CPU) argument is uploaded to the device of the weights.  weights: lpips.load_weights / lpips.from_tensors.  Returns a device tensor:
    each pair's value (0-dim for one pair: summary.py:68) or, with return_map, the unclipped map [..., H, W] (summary.py:66 before its
    clip).  Nothing is synchronised.  There is no CPU fallback."""
    s0, s1 = tuple(np.shape(img0)), tuple(np.shape(img1))
    if s0 != s1:
        raise ValueError(f"compute_lpips: the images differ in shape: {s0} vs {s1}")
    if len(s0) not in (3, 4) or s0[-1] != 3:
        raise ValueError(f"compute_lpips: need [H, W, 3] or [n, H, W, 3] images, got shape {s0}")
    from . import ops
    return ops.lpips(ops.as_f32(img0, weights.device), ops.as_f32(img1, weights.device), weights, return_map=return_map)


def save_img(img, pth, to8b=True):
    """rnerf/utils.py:474-488: a PNG of `img` ([H, W] or [H, W, C]); with to8b the values are clipped to [0, 1] and scaled by 255, the
    cast to uint8 truncating.  Accepts a device tensor (read back here) or a numpy array."""
    from PIL import Image
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    with open(pth, "wb") as imgout:
        if to8b:
            Image.fromarray(np.array((np.clip(img, 0., 1.) * 255.).astype(np.uint8))).save(imgout, "PNG")
        else:
            Image.fromarray(np.array(img)).save(imgout, "PNG")


def learning_rate_decay(step, lr_init, lr_final, max_steps, lr_delay_steps=0, lr_delay_mult=1, lr_start_steps=0):
    """rnerf/utils.py:490-528."""
    if lr_delay_steps > 0:
        delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0), 1))
    else:
        delay_rate = 1.0
    start_rate = min(max(step - lr_start_steps, 0), 1)
    t = min(max(max(step - lr_start_steps, 0) / (max_steps - lr_start_steps), 0), 1)
    log_lerp = math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return start_rate * delay_rate * log_lerp


def render_image(render_fn: Callable, rays: Rays, rng, normalize_disp: bool, chunk: int = 8192, model=None):
    """rnerf/utils.py:331-389.  `render_fn(key_0, key_1, chunk_rays)` -> (ret, loss_sp); the fine tuple ret[-1] is kept.

    rays: Rays of [H, W, ...] tensors.  Returns (rgb [H,W,3], dist [H,W,1], acc [H,W,1]).  The same key pair is used for
    every chunk (:350).  With `model=` the chunks are software-pipelined (march of chunk k+1 beside the MLP of chunk k) and
    render_fn must accept `path=`.  There is no device padding/sharding here: one process renders on one GPU; multi-GPU eval gives
    each rank a contiguous block of rows and needs no collective (samplenerfro_amd.distributed.render_image_sharded).
    """
    height, width = rays[0].shape[:2]
    num_rays = height * width
    rays = namedtuple_map(lambda r: None if r is None else r.reshape((num_rays, -1)), rays)
    _unused, key_0, key_1 = prng.split(rng, 3)
    results = []
    if model is not None:
        # pipelined form: `render_fn(key_0, key_1, chunk_rays, path=handle)`; the march of chunk k+1 runs on the model's side
        # stream while chunk k is in its MLP phase (NerfModel.prefetch_path)
        starts = list(range(0, num_rays, chunk))
        get = lambda i: namedtuple_map(lambda r: None if r is None else r[i:i + chunk], rays)
        nxt_rays = get(starts[0]); handle = model.prefetch_path(nxt_rays, sync_inputs=True)
        for k, i in enumerate(starts):
            cur_rays, cur_handle = nxt_rays, handle
            if k + 1 < len(starts):
                nxt_rays = get(starts[k + 1]); handle = model.prefetch_path(nxt_rays, sync_inputs=False)
            results.append(render_fn(key_0, key_1, cur_rays, path=cur_handle)[0][-1])
    else:
        for i in range(0, num_rays, chunk):
            chunk_rays = namedtuple_map(lambda r: None if r is None else r[i:i + chunk], rays)
            chunk_results = render_fn(key_0, key_1, chunk_rays)[0][-1]
            results.append(chunk_results)
    rgb, distance, acc, _trans, _trans_rgb_bkgd = [torch.cat(r, dim=0) for r in zip(*results)]
    if normalize_disp:
        distance = (distance - distance.min()) / (distance.max() - distance.min())
    return (rgb.reshape((height, width, -1)), distance.reshape((height, width, -1)), acc.reshape((height, width, -1)))
