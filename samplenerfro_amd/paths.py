"""Bent-path diagnostics: where a view's rays refract and how strongly, and the paths of chosen pixels drawn from four directions.

The reference's extract_mesh.py renders one view, pickles the bent path of one pixel (:178-223), draws it with plt_utils.plot_path (:225)
and exits; eval.py:173,195 carries the per-pixel form commented out (`pred_mask = any(|idx_grad| > 1e-3 along the path)`, mask_{idx}.png).
Here the march's records never leave the device: `view_maps` reduces them per ray chunk by chunk (rnerf_path_summary), `plot_paths` draws
polylines as finished bytes (rnerf_path_plot; no matplotlib, no perspective, no text), `trace_pixels` / `save_ray_pkl` give the reference's
pickle for single pixels.  evaluate.evaluate(path_maps=True) writes the maps of every view.
"""
from __future__ import annotations

import math
import os
import pickle
from typing import Optional

import numpy as np
import torch

from . import ops, prng
from .utils import Rays

GRAD_EPS = 1e-3            # eikonal_utils.py:35, eval.py:173
VIEWS = (("top", 90, 0), ("right", 0, 0), ("front", 0, 90), ("free", 30, -60))      # plot_path:86 (name, elevation, azimuth in degrees)
MIN_PLOT_SIZE = 8


def march(model, variables, rays: Rays, annealed_alpha: float = 1.0):
    """The march model.forward runs for the model's stage, with the IoR record and nothing after it (no MLP is evaluated): ops.march for
    radiance* / ior*, ops.march_all (so3_mlp bends the gradient) for all*.  rays: Rays of [B, 3] origins / viewdirs -> (pd, dr, ior), each
    [num_samples, B, 4]."""
    from . import models
    o, v = rays.origins, rays.viewdirs
    if o.dim() != 2 or o.shape[-1] != 3:
        raise ValueError("paths.march: rays.origins must be [B, 3]")
    if model.stage.startswith("all"):
        so3 = model._flat(variables, "so3_mlp", models.SO3_MLP_SHAPES).detach()
        return ops.march_all(model.table, model.spec, so3, o, v, model.near, model.far, model.num_samples, annealed_alpha, want_ior=True)
    pd, dr, ior, _ = ops.march(model.table, model.spec, o, v, model.near, model.far, model.num_samples, want_ior=True)
    return pd, dr, ior


def summarize(pd: torch.Tensor, dr: torch.Tensor, ior: torch.Tensor, grad_eps: float = GRAD_EPS) -> dict:
    """Records [N, B, 4] -> {"nodes": int32 [B], the number of nodes with |grad n| > grad_eps; "first", "last": int32 [B], the first and
    the last such node, -1 if none; "bend": float32 [B], |d_last - d_first| = 2 sin(theta / 2) of the total deflection theta; "optical":
    float32 [B], sum over the segments of (n - 1) x length}."""
    nodes, maps = ops.path_summary(pd, dr, ior, grad_eps)
    return {"nodes": nodes[0], "first": nodes[1], "last": nodes[2], "bend": maps[0], "optical": maps[1]}


def view_maps(model, variables, rays: Rays, chunk: int = 8192, annealed_alpha: float = 1.0, grad_eps: float = GRAD_EPS) -> dict:
    """summarize for a whole view.  rays: Rays of [H, W, 3] tensors (evaluate.device_views) -> the five maps of summarize as [H, W] tensors
    and "refracted" (bool [H, W], nodes > 0).  The view is marched `chunk` rays at a time and no path record outlives its chunk: a chunk
    of 8192 rays holds 0.6 GB of records at 1536 nodes."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"view_maps: chunk must be >= 1, got {chunk}")
    H, W = (int(s) for s in rays.origins.shape[:2])
    n = H * W
    o, v = rays.origins.reshape(n, 3), rays.viewdirs.reshape(n, 3)
    dev = o.device
    nodes = torch.empty((3, n), dtype=torch.int32, device=dev)
    maps = torch.empty((2, n), dtype=torch.float32, device=dev)
    for s in range(0, n, chunk):
        pd, dr, ior = march(model, variables, Rays(o[s:s + chunk].contiguous(), None, v[s:s + chunk].contiguous(), None), annealed_alpha)
        nd, mp = ops.path_summary(pd, dr, ior, grad_eps)
        nodes[:, s:s + chunk] = nd
        maps[:, s:s + chunk] = mp
        del pd, dr, ior
    out = {"nodes": nodes[0], "first": nodes[1], "last": nodes[2], "bend": maps[0], "optical": maps[1]}
    out = {k: t.reshape(H, W) for k, t in out.items()}
    out["refracted"] = out["nodes"] > 0
    return out


def visualize_maps(maps: dict) -> dict:
    """-> {"mask": float32 [H, W], 1 where a node of the ray refracts (eval.py:173's pred_mask); "bend", "optical": [H, W, 3], the map
    through vis.visualize_depth(curve_fn="identity", acc=refracted): turbo between the view's smallest and largest value, white where the
    ray does not refract — a view without refraction is white."""
    from . import vis
    acc = maps["refracted"].to(torch.float32)
    return {"mask": acc,
            "bend": vis.visualize_depth(maps["bend"], acc, curve_fn="identity"),
            "optical": vis.visualize_depth(maps["optical"], acc, curve_fn="identity")}


def _pixel_indices(pixels, H: int, W: int) -> np.ndarray:
    px = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    if px.shape[0] < 1:
        raise ValueError("paths: no pixel given")
    bad = (px[:, 0] < 0) | (px[:, 0] >= H) | (px[:, 1] < 0) | (px[:, 1] >= W)
    if bad.any():
        raise ValueError(f"paths: pixel (row, col) = {tuple(px[bad][0])} lies outside the {H} x {W} view")
    return px


def trace_pixels(model, variables, rays: Rays, pixels, rng, transform=None, annealed_alpha: float = 1.0) -> list:
    """The dict extract_mesh.py:216-223 pickles, for each (row, col) of `pixels`.  rays: Rays of [H, W, 3] tensors; rng: the render key
    as utils.render_image and evaluate take it.  -> one {"ray_pos", "ray_dir", "idx_grad": float32 numpy [1, N, 3] (position, direction,
    grad n of every node); "transform": as given (the view's camera-to-world there); "ray_pos_c": [1, N_c, 3], the nodes the coarse level
    samples — the jitter model.forward draws from the same key} per pixel."""
    H, W = (int(s) for s in rays.origins.shape[:2])
    px = _pixel_indices(pixels, H, W)
    idx = torch.from_numpy(px[:, 0] * W + px[:, 1]).to(rays.origins.device)
    o = rays.origins.reshape(H * W, 3)[idx].contiguous()
    v = rays.viewdirs.reshape(H * W, 3)[idx].contiguous()
    pd, dr, ior = march(model, variables, Rays(o, None, v, None), annealed_alpha)
    _unused, key_0, _key_1 = prng.split(np.asarray(rng, np.uint32), 3)          # utils.render_image
    key, _ = prng.split(np.asarray(key_0, np.uint32))                            # NerfModel.forward
    jitter = np.asarray(model.make_jitter(key), np.int64)
    pos = pd[:, :, :3].permute(1, 0, 2).cpu().numpy()
    dirs = dr[:, :, :3].permute(1, 0, 2).cpu().numpy()
    grad = ior[:, :, 1:4].permute(1, 0, 2).cpu().numpy()
    return [{"ray_pos": np.ascontiguousarray(pos[i:i + 1]), "ray_dir": np.ascontiguousarray(dirs[i:i + 1]),
             "idx_grad": np.ascontiguousarray(grad[i:i + 1]), "transform": transform,
             "ray_pos_c": np.ascontiguousarray(pos[i:i + 1][:, jitter])} for i in range(px.shape[0])]


def save_ray_pkl(out_dir: str, img_idx: int, row: int, col: int, rec: dict) -> str:
    """extract_mesh.py:216: ray_{img_idx:03d}_{row:03d}_{col:03d}.pkl in out_dir -> its path."""
    path = os.path.join(out_dir, f"ray_{int(img_idx):03d}_{int(row):03d}_{int(col):03d}.pkl")
    with open(path, "wb") as f:
        pickle.dump({k: rec[k] for k in ("ray_pos", "ray_dir", "idx_grad", "transform", "ray_pos_c")}, f)
    return path


def view_matrices(center, side: float, size: int, views=VIEWS) -> np.ndarray:
    """float64 [len(views), 2, 4]: per (name, elevation, azimuth) the rows (u, v) of an orthographic view along f = (cos e cos a,
    cos e sin a, sin e) with right = (-sin a, cos a, 0) and up = f x right: u = scale right . (x - center) + size / 2, v = -scale up .
    (x - center) + size / 2, scale = (size - 1) / (sqrt(3) side) — the cube of that side around center fits into every view."""
    c = np.asarray(center, np.float64).reshape(3)
    scale = (float(size) - 1.0) / (math.sqrt(3.0) * float(side))
    out = np.zeros((len(views), 2, 4), np.float64)
    for i, (_name, elev, azim) in enumerate(views):
        e, a = math.radians(elev), math.radians(azim)
        f = np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)])
        right = np.array([-math.sin(a), math.cos(a), 0.0])
        up = np.cross(f, right)
        out[i, 0, :3] = scale * right
        out[i, 0, 3] = -scale * float(right @ c) + size / 2
        out[i, 1, :3] = -scale * up
        out[i, 1, 3] = scale * float(up @ c) + size / 2
    return out


def ray_colours(R: int) -> np.ndarray:
    """plot_path:38-40: uint8 [R, 3], colour j = ((j % sz + 1) / sz, (j // sz + 1) / sz, 0) x 255 truncated, sz = ceil(sqrt(R))."""
    R = int(R)
    if R < 1:
        raise ValueError(f"ray_colours: need at least one ray, got {R}")
    sz = int(math.ceil(math.sqrt(R)))
    j = np.arange(R)
    c = np.stack([(j % sz + 1) / sz, (j // sz + 1) / sz, np.zeros(R)], axis=-1)
    return (c * 255.0).astype(np.uint8)


def _ray_indices(rays, B: int) -> np.ndarray:
    if isinstance(rays, torch.Tensor):
        rays = rays.detach().cpu().numpy()
    r = np.asarray(rays)
    if r.ndim != 1 or r.size < 1 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("plot_paths: rays must be a non-empty 1-D sequence of integer ray indices")
    r = r.astype(np.int64)
    if r.min() < 0 or r.max() >= B:
        raise ValueError(f"plot_paths: ray indices must lie in [0, {B}), got {int(r.min())} .. {int(r.max())}")
    return r.astype(np.int32)


def plot_paths(pd: torch.Tensor, ior: Optional[torch.Tensor], rays, size: int = 512, frame: str = "paths", box=None,
               shadow: bool = True, grad_eps: float = GRAD_EPS) -> torch.Tensor:
    """plt_utils.plot_path's four pictures -> uint8 [4, size, size, 3] on pd's device, in the order of VIEWS.  pd, ior: records
    [N, B, 4] (ior None: no markers on the refracting nodes); rays: the indices of the rays to draw, coloured by ray_colours; box: None
    or (min x, y, z, max x, y, z), e.g. the grid's nmin + nmax, drawn in red.  frame "paths": centre = the mean of the drawn positions,
    side = their largest extent (plot_path:32-35; one small read-back); "grid": the box's centre and largest side.  shadow: the polyline
    again on the plane z = centre_z - side / 2 (plot_path:54)."""
    if pd.dim() != 3 or int(pd.shape[2]) != 4:
        raise ValueError(f"plot_paths: pd must be [num_nodes, B, 4], got {tuple(pd.shape)}")
    size = int(size)
    if size < MIN_PLOT_SIZE:
        raise ValueError(f"plot_paths: size must be >= {MIN_PLOT_SIZE}, got {size}")
    if frame not in ("paths", "grid"):
        raise ValueError(f"plot_paths: frame must be 'paths' or 'grid', got {frame!r}")
    if frame == "grid" and box is None:
        raise ValueError("plot_paths: frame='grid' needs the box")
    r = _ray_indices(rays, int(pd.shape[1]))
    bx = None if box is None else np.asarray(box, np.float64).reshape(6)
    dev = pd.device
    rt = torch.from_numpy(r).to(dev)
    if frame == "paths":
        pos = pd[:, rt.long(), :3].reshape(-1, 3).cpu().numpy().astype(np.float64)
        center, side = pos.mean(axis=0), float((pos.max(axis=0) - pos.min(axis=0)).max())
    else:
        center, side = 0.5 * (bx[:3] + bx[3:]), float((bx[3:] - bx[:3]).max())
    if not side > 0.0:
        side = 1.0                                       # a single point (or NaN positions): any finite scale
    floor_z = float(center[2] - side * 0.5) if shadow else float("nan")
    rgb = torch.from_numpy(ray_colours(r.size)).to(dev)
    return ops.path_plot(pd, ior, rt, rgb, view_matrices(center, side, size), size, box=bx, floor_z=floor_z, grad_eps=grad_eps)


def write_plots(out_dir: str, panels: torch.Tensor, views=VIEWS) -> list:
    """{out_dir}/top.png, right.png, front.png, free.png (plot_path:86-89) from plot_paths' panels -> the paths written."""
    from PIL import Image
    if panels.dim() != 4 or int(panels.shape[0]) != len(views) or panels.dtype != torch.uint8:
        raise ValueError(f"write_plots: need uint8 [{len(views)}, size, size, 3] panels, got {panels.dtype} {tuple(panels.shape)}")
    os.makedirs(out_dir, exist_ok=True)
    host = panels.cpu().numpy()
    names = []
    for (name, _e, _a), img in zip(views, host):
        names.append(os.path.join(out_dir, f"{name}.png"))
        Image.fromarray(img).save(names[-1], "PNG")
    return names
