"""Depth visualisations: rnerf/vis.py's call surface on the device (rnerf_vis_depth, rnerf_vis_normals; csrc/vis.hip), without JAX,
jax.scipy or matplotlib.  Every function returns float32 device tensors and synchronises nothing; numpy arrays and CPU tensors are
uploaded to the device of the other argument, or to the current device.  There is no CPU fallback.

visualize_suite(depth, acc) is what eval.py:175 computes for every view; evaluate.evaluate(vis_suite=True) calls it."""
from __future__ import annotations

import math

import torch

from . import _lib, ops

CURVES = tuple(_lib.VIS_CURVES)          # the choices the reference's docstring names (vis.py:62-65), "neg_log" its default


def _bound(v):
    """`near or ...` (vis.py:90-91): None and 0 are "automatic"."""
    return None if v is None or float(v) == 0.0 or math.isnan(float(v)) else float(v)


def sinebow(h):
    """vis.py:23-26: a cyclic and uniform colour map, sin(pi x)^2 at 3/6 - h, 5/6 - h, 7/6 - h -> [..., 3].  The kernel has this built in
    for modulus > 0; this is the same map for use as a `colormap`."""
    h = ops.as_f32(h, ops.device_of(h))
    f = lambda x: torch.sin(math.pi * x) ** 2
    return torch.stack([f(3 / 6 - h), f(5 / 6 - h), f(7 / 6 - h)], -1)


def depth_to_normals(depth):
    """vis.py:34-42: `depth` [H, W] taken as orthographic -> normals [H, W, 3] (true 3 x 3 convolutions with zero padding)."""
    d = ops.as_f32(depth, ops.device_of(depth))
    return ops.vis_normals(d, None, scaling=1.0, want_rgb=False, want_normals=True)[1]


def visualize_depth(depth, acc=None, near=None, far=None, ignore_frac=0, curve_fn="neg_log", modulus=0, colormap=None):
    """vis.py:45-111 -> rgb [H, W, 3].

    depth [H, W]; acc [H, W] in [0, 1] (None: ones); near / far: None or 0 = automatic, from the depths that span the middle of acc with
    ignore_frac (in [0, 0.5)) of it ignored at either end.  curve_fn: one of CURVES by name — "neg_log" (-log(x + eps), the reference's
    default), "identity", "reciprocal" (1 / (x + eps)), "log" (log(x + eps)); Python callables are not supported.  modulus > 0 wraps the
    curved depth.  colormap: None = turbo (modulus == 0) or sinebow (modulus > 0), applied in the kernel; a callable maps the kernel's
    value plane (a device tensor [H, W]) to [H, W, >= 3] and is blended with acc here."""
    if not isinstance(curve_fn, str) or curve_fn not in _lib.VIS_CURVES:
        if callable(curve_fn):
            raise TypeError(f"visualize_depth: curve_fn is chosen by name, one of {list(CURVES)}; a callable cannot run in the kernel")
        raise ValueError(f"visualize_depth: curve_fn must be one of {list(CURVES)}, got {curve_fn!r}")
    if colormap is not None and not callable(colormap):
        raise TypeError("visualize_depth: colormap must be None or a callable on a device tensor")
    dev = ops.device_of(depth, acc)
    d, a = ops.as_f32(depth, dev), ops.as_f32(acc, dev)
    kw = dict(near=_bound(near), far=_bound(far), ignore_frac=float(ignore_frac), curve=curve_fn, modulus=float(modulus))
    if colormap is None:
        return ops.vis_depth(d, a, **kw)[0]
    value = ops.vis_depth(d, a, want_rgb=False, want_value=True, **kw)[1]
    colour = colormap(value)
    if not isinstance(colour, torch.Tensor) or colour.dim() != 3 or tuple(colour.shape[:2]) != tuple(d.shape) or int(colour.shape[2]) < 3:
        raise ValueError(f"visualize_depth: colormap must map the [H, W] value tensor to a tensor [H, W, >= 3], got {type(colour).__name__} "
                         f"{tuple(getattr(colour, 'shape', ()))}")
    colour = colour[:, :, :3].to(device=dev, dtype=torch.float32)
    w = torch.ones_like(d) if a is None else a
    w = torch.where(torch.isnan(d), torch.zeros_like(w), w)[:, :, None]
    return colour * w + (1 - w)


def visualize_normals(depth, acc, scaling=None):
    """vis.py:114-132 -> rgb [H, W, 3]: the fake normals of `depth`, scaled to be isotropic unless `scaling` is given, as colours, blended
    with acc unless it is None."""
    dev = ops.device_of(depth, acc)
    return ops.vis_normals(ops.as_f32(depth, dev), ops.as_f32(acc, dev), scaling=None if scaling is None else float(scaling))[0]


def visualize_suite(depth, acc):
    """vis.py:135-142 -> {"depth", "depth_mod" (modulus 0.1), "depth_normals"}, each [H, W, 3].  Seven launches."""
    dev = ops.device_of(depth, acc)
    d, a = ops.as_f32(depth, dev), ops.as_f32(acc, dev)
    return {"depth": ops.vis_depth(d, a)[0], "depth_mod": ops.vis_depth(d, a, modulus=0.1)[0], "depth_normals": ops.vis_normals(d, a)[0]}
