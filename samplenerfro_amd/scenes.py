"""Synthetic refractive scenes with ground truth: multi-view images that are physically consistent with an IoR grid.

The reference trains on Blender Cycles renders named `*_skydome-bkgd_no-partial-reflect_cycles`: a refractive object in front of an
environment, no partial reflection.  That image formation is what the model family represents — an eikonal march through the grid, a
background that depends on the last bent direction only (`bkgd_mlp(dir_last)`), a participating medium in front of it — so the same march
renders the ground truth here: `ops.scene_trace` (rnerf_scene_trace: where every ray of a frame ends up, no path records) and
`ops.scene_shade` (rnerf_scene_shade: a cube-map environment behind a grey medium, K x K sub-samples per pixel).  DESIGN.md 3.19.

Host side (numpy): the environment (`cube_from_function`, `procedural_env`), the cameras (`pose_spherical`, `orbit_cameras`) and the
Blender-layout writer (`write_scene`), whose output `datasets.get_dataset`, `datasets.load_masks` and `grid.load_mesh_pkl` open as any
other scene.  Partial reflection, Fresnel terms, per-channel absorption and seamless filtering across cube edges are not modelled.
"""
from __future__ import annotations

import json
import os
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import grid as grid_mod
from . import mesh_mask, ops, utils, voxelize
from ._lib import Grid

FACES = ("+x", "-x", "+y", "-y", "+z", "-z")      # face index of rnerf_scene_shade


# ---- the environment ----------------------------------------------------------------------------------------------------------------------
def cube_directions(E: int) -> np.ndarray:
    """Unit directions float64 [6, E, E, 3] of the texel centres env[face][v][u] of rnerf_scene_shade's lookup: on face (axis, sign) the
    major component is sign, the face coordinates (s, t) = ((u + 0.5) 2 / E - 1, (v + 0.5) 2 / E - 1) are (y, z), (z, x), (x, y)."""
    E = int(E)
    if E < 1:
        raise ValueError("cube_directions: E must be >= 1")
    c = (np.arange(E, dtype=np.float64) + 0.5) * 2.0 / E - 1.0
    t, s = np.meshgrid(c, c, indexing="ij")            # [v, u]
    out = np.empty((6, E, E, 3), np.float64)
    for face in range(6):
        axis, sign = face // 2, 1.0 - 2.0 * (face % 2)
        out[face, ..., axis] = sign
        out[face, ..., (axis + 1) % 3] = s
        out[face, ..., (axis + 2) % 3] = t
    return out / np.linalg.norm(out, axis=-1, keepdims=True)


def cube_from_function(fn: Callable[[np.ndarray], np.ndarray], E: int) -> np.ndarray:
    """The cube map float32 [6, E, E, 3] of `fn`, which maps unit directions float64 [..., 3] to rgb [..., 3], sampled at the texel
    centres (cube_directions).  An equirectangular panorama goes through here: fn looks it up."""
    rgb = np.asarray(fn(cube_directions(E)), np.float64)
    if rgb.shape != (6, int(E), int(E), 3):
        raise ValueError(f"cube_from_function: fn must return [..., 3] for [..., 3] directions, got {rgb.shape}")
    return np.ascontiguousarray(rgb.astype(np.float32))


def procedural_env(E: int, seed: int = 0) -> np.ndarray:
    """A seeded environment with structure at every scale that refraction visibly displaces: a smooth sky gradient along z (up, as in
    pose_spherical), a checker band around the horizon and a few coloured blobs.  float32 [6, E, E, 3] in [0, 1]; the same bytes for the
    same (E, seed)."""
    rng = np.random.default_rng(int(seed))
    ground, horizon, zenith = rng.uniform(0.15, 0.45, 3), rng.uniform(0.65, 0.95, 3), rng.uniform(0.1, 0.5, 3)
    zenith[2] = rng.uniform(0.7, 1.0)
    phase = rng.uniform(0.0, 2.0 * np.pi)
    n_blobs = 5
    centres = rng.standard_normal((n_blobs, 3))
    centres /= np.linalg.norm(centres, axis=-1, keepdims=True)
    colours = rng.uniform(0.0, 1.0, (n_blobs, 3))
    widths = rng.uniform(0.02, 0.08, n_blobs)

    def fn(d):
        z = d[..., 2:3]
        up = np.clip(z, 0.0, 1.0) ** 0.5
        down = np.clip(-z, 0.0, 1.0) ** 0.5
        rgb = horizon * (1.0 - up - down) + zenith * up + ground * down
        az = np.arctan2(d[..., 1], d[..., 0]) + phase
        cell = (np.floor(az / (2.0 * np.pi) * 24.0) + np.floor((d[..., 2] + 0.3) / 0.15)) % 2.0
        band = (np.abs(d[..., 2]) < 0.3)[..., None]
        rgb = np.where(band, np.where(cell[..., None] > 0.5, 0.9, 0.1) * (0.5 + 0.5 * rgb), rgb)
        for c, col, w in zip(centres, colours, widths):
            a = np.exp(-(1.0 - d @ c) / w)[..., None]
            rgb = rgb * (1.0 - a) + col * a
        return np.clip(rgb, 0.0, 1.0)

    return cube_from_function(fn, E)


# ---- the cameras --------------------------------------------------------------------------------------------------------------------------
def pose_spherical(theta: float, phi: float, radius: float) -> np.ndarray:
    """rnerf/math_utils.py:42-66: the camera on the sphere of `radius` at azimuth theta and elevation phi (degrees), looking at the
    origin, z up.  float32 [4, 4], the products taken in float32 as there."""
    f = np.float32
    trans_t = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]], dtype=f)
    p, t = phi / 180. * np.pi, theta / 180. * np.pi
    rot_phi = np.array([[1, 0, 0, 0], [0, np.cos(p), -np.sin(p), 0], [0, np.sin(p), np.cos(p), 0], [0, 0, 0, 1]], dtype=f)
    rot_theta = np.array([[np.cos(t), 0, -np.sin(t), 0], [0, 1, 0, 0], [np.sin(t), 0, np.cos(t), 0], [0, 0, 0, 1]], dtype=f)
    c2w = rot_theta @ (rot_phi @ trans_t)
    return np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=f) @ c2w


def orbit_cameras(n: int, radius: float, phis: Sequence[float], seed: Optional[int] = None) -> np.ndarray:
    """n poses float32 [n, 4, 4] around the origin: thetas evenly spaced over the circle (seed: rotated by one seeded offset, so that a
    held-out split does not repeat the training azimuths), elevations cycling through `phis` (degrees, negative = above the horizon as in
    the reference's render paths)."""
    phis = [float(p) for p in phis]
    if n < 1 or not phis:
        raise ValueError("orbit_cameras: need n >= 1 and at least one elevation")
    off = 0.0 if seed is None else float(np.random.default_rng(int(seed)).uniform(0.0, 360.0 / n))
    return np.stack([pose_spherical(-180.0 + off + 360.0 * i / n, phis[i % len(phis)], radius) for i in range(n)], axis=0)


# ---- one view -----------------------------------------------------------------------------------------------------------------------------
def default_n_inside(table: torch.Tensor, spec: Grid) -> float:
    """The midpoint of the smallest and the largest n over the grid's own entries.  A brick table of a grid with an odd dimension is
    padded with zeroed entries that no lookup reads: they are cut off (the bricks viewed as [2 bx, 2 by, 2 bz] and sliced to the grid; no
    index gather, so a 512^3 table is two reductions)."""
    from ._lib import TABLE_LAYOUTS
    dx, dy, dz = (int(v) for v in spec.dims)
    if spec.layout == TABLE_LAYOUTS["reference"]:
        n = table.reshape(-1, 4)[:, 0]
    else:                                               # entry (x, y, z) sits at brick (x >> 1, y >> 1, z >> 1), place (x & 1, y & 1, z & 1)
        bx, by, bz = (dx + 1) // 2, (dy + 1) // 2, (dz + 1) // 2
        n = table.reshape(bx, by, bz, 2, 2, 2, 4)[..., 0].permute(0, 3, 1, 4, 2, 5).reshape(2 * bx, 2 * by, 2 * bz)[:dx, :dy, :dz]
    return 0.5 * (float(n.min()) + float(n.max()))


def render_view(table: torch.Tensor, spec: Grid, env, camtoworld, H: int, W: int, *, focal: Optional[float] = None, cam_mat=None, near: float,
                far: float, num_nodes: int, supersample: int = 2, n_inside: Optional[float] = None, grad_eps: float = 1e-3, sigma: float = 0.0,
                albedo=(0.0, 0.0, 0.0), pixel_center: bool = False, chunk: int = 1 << 18, device=None) -> dict:
    """The ground-truth image of one camera -> {"rgb": float32 [H, W, 3], "trans": float32 [H, W], "mask": uint8 [H, W]} on the device.

    The rays are those of the K = supersample times finer camera (ops.generate_rays with focal K, or fx, fy, cx, cy each times K;
    pixel_center as the loader of the scene will use it), traced in chunks of whole fine rows (`chunk` rays at most, one row at least)
    and shaded once.  env: float32 [6, E, E, 3] (numpy or tensor).  sigma: extinction per unit length of the medium inside the object
    (nodes with n > n_inside; None: default_n_inside), albedo its colour; mask: pixels a refracting node was met on (|grad n| > grad_eps)."""
    if (focal is None) == (cam_mat is None):
        raise ValueError("render_view: give focal= (Blender camera) or cam_mat= (OpenCV camera)")
    H, W, K = int(H), int(W), int(supersample)
    if H < 1 or W < 1 or K < 1:
        raise ValueError("render_view: need H, W and supersample >= 1")
    dev = ops.device_of(table, device=device)
    if cam_mat is None:
        cam = dict(focal=float(focal) * K)
    else:
        cam = dict(cam_mat=[[float(cam_mat[0][0]) * K, 0.0, float(cam_mat[0][2]) * K], [0.0, float(cam_mat[1][1]) * K, float(cam_mat[1][2]) * K], [0.0, 0.0, 1.0]])
    if n_inside is None:
        n_inside = default_n_inside(table, spec)
    c2w = camtoworld.detach().cpu().numpy() if isinstance(camtoworld, torch.Tensor) else np.asarray(camtoworld)
    fh, fw = H * K, W * K
    with torch.cuda.device(dev):
        rows = max(1, int(chunk) // fw)
        if rows >= fh:
            o, _, v = ops.generate_rays(c2w, fh, fw, dev, pixel_center=pixel_center, **cam)
            exit_dir, counts = ops.scene_trace(table, spec, o, v, near, far, num_nodes, n_inside=n_inside, grad_eps=grad_eps)
        else:
            exit_dir = torch.empty((fh * fw, 4), dtype=torch.float32, device=dev)
            counts = torch.empty((2, fh * fw), dtype=torch.int32, device=dev)
            for r0 in range(0, fh, rows):
                r1 = min(fh, r0 + rows)
                o, _, v = ops.generate_rays(c2w, fh, fw, dev, pixel_center=pixel_center, rows=(r0, r1), **cam)
                e, c = ops.scene_trace(table, spec, o, v, near, far, num_nodes, n_inside=n_inside, grad_eps=grad_eps)
                exit_dir[r0 * fw:r1 * fw] = e
                counts[:, r0 * fw:r1 * fw] = c          # a chunk's two rows of counts [2, B] are not contiguous in the frame's
        step_len = float(np.float32((float(far) - float(near)) / (int(num_nodes) - 1)))
        rgb, trans, mask = ops.scene_shade(exit_dir, counts, H, W, K, ops.as_f32(env, dev).contiguous(), step_len=step_len, sigma=sigma, albedo=albedo)
    return {"rgb": rgb, "trans": trans, "mask": mask}


# ---- a whole scene on disk ----------------------------------------------------------------------------------------------------------------
SPLITS = ("train", "val", "test")


def write_scene(directory: str, raw_grid, *, extent: float, env, n_train: int, n_val: int, n_test: int, H: int, W: int, camera_angle_x: float,
                radius: float = 4.0, phis: Sequence[float] = (-30.0, -10.0, -50.0), near: float = 2.0, far: float = 6.0, num_nodes: int = 768,
                supersample: int = 2, sigma: float = 0.0, albedo=(0.0, 0.0, 0.0), config: str = "synthetic", kernel_size: int = 3,
                kernel_sigma: float = 1.0, layout: str = "bricks", seed: int = 0, device=None, **flag_overrides) -> dict:
    """Render and write a Blender-layout scene that datasets.get_dataset opens without change.

    raw_grid: the voxeliser's output (values in [1, 1.33], [G, G, G] or [G^3, 1], x slowest) on the cube [-extent, extent]^3.  It is
    written to voxelize/mesh.pkl (voxelize.save_mesh_pkl) and prepared as a training run prepares it (grid.prepare_grid: the IoR scale
    `config` selects, the kernel_size / kernel_sigma prefilter), so the rendered object is the one a model built from the scene marches
    through.  Cameras: orbit_cameras(n, radius, phis, seed) per split, the splits' azimuths offset against each other.

    Written: transforms_{train,val,test}.json (camera_angle_x, frames with file_path ./<split>/r_<i> and transform_matrix),
    <split>/r_<i>.png (RGBA, alpha 255, the quantisation of utils.save_img) and <split>/mask_r_<i>.png (mesh_mask.mask_file_name; 0 / 255).

    -> {"flags": utils.default_flags(...) describing the scene (data_dir, dataset, factor 0, white_bkgd False, near, far, use_pixel_centers
    True, config, voxel_grid, kernel_size, kernel_sigma, then flag_overrides), "focal", "n_inside", <split>: {"images": uint8 [n, H, W, 4],
    "masks": uint8 [n, H, W], "camtoworlds": float32 [n, 4, 4], "trans": float32 [n, H, W]}}."""
    from PIL import Image
    dev = ops.device_of(device=device)
    data = raw_grid.detach().cpu().numpy() if isinstance(raw_grid, torch.Tensor) else np.asarray(raw_grid)
    G = int(round(data.size ** (1.0 / 3.0)))
    if G ** 3 != data.size:
        raise ValueError(f"write_scene: raw_grid must hold G^3 voxels, got {data.size}")
    ndim, nmin, nmax = [G] * 3, [-float(extent)] * 3, [float(extent)] * 3
    os.makedirs(os.path.join(directory, "voxelize"), exist_ok=True)
    voxelize.save_mesh_pkl(os.path.join(directory, "voxelize", "mesh.pkl"), data.reshape(-1, 1), extent=float(extent), num_voxels=G)
    g = grid_mod.prepare_grid(data.reshape(-1, 1), ndim, config, int(kernel_size), float(kernel_sigma), dev)
    spec = Grid.make(ndim, nmin, nmax, layout)
    table = ops.grid_build_table(g, spec)
    n_inside = default_n_inside(table, spec)
    focal = .5 * W / np.tan(.5 * float(camera_angle_x))                  # what the loader computes (datasets.py:368-369)
    env_t = ops.as_f32(env, dev).contiguous()
    out = {"focal": focal, "n_inside": n_inside}
    for k, (split, n) in enumerate(zip(SPLITS, (n_train, n_val, n_test))):
        poses = orbit_cameras(n, radius, phis, seed=int(seed) * 3 + k) if n > 0 else np.zeros((0, 4, 4), np.float32)
        os.makedirs(os.path.join(directory, split), exist_ok=True)
        images, masks, trans, frames = [], [], [], []
        for i in range(n):
            view = render_view(table, spec, env_t, poses[i], H, W, focal=focal, near=near, far=far, num_nodes=num_nodes, supersample=supersample,
                               n_inside=n_inside, sigma=sigma, albedo=albedo, pixel_center=True, device=dev)
            file_path = f"./{split}/r_{i}"
            rgba = torch.cat([view["rgb"], torch.ones_like(view["rgb"][..., :1])], dim=-1)
            utils.save_img(rgba, os.path.join(directory, file_path + ".png"))
            m = view["mask"].cpu().numpy()
            Image.fromarray(m).save(os.path.join(directory, mesh_mask.mask_file_name(file_path, "blender")), "PNG")
            images.append((np.clip(rgba.cpu().numpy(), 0., 1.) * 255.).astype(np.uint8))      # save_img's rule: the bytes in the PNG
            masks.append(m); trans.append(view["trans"].cpu().numpy())
            frames.append({"file_path": file_path, "transform_matrix": poses[i].astype(np.float64).tolist()})
        with open(os.path.join(directory, f"transforms_{split}.json"), "w") as fp:
            json.dump({"camera_angle_x": float(camera_angle_x), "frames": frames}, fp, indent=1)
        out[split] = {"images": np.stack(images) if images else np.zeros((0, H, W, 4), np.uint8),
                      "masks": np.stack(masks) if masks else np.zeros((0, H, W), np.uint8),
                      "trans": np.stack(trans) if trans else np.zeros((0, H, W), np.float32), "camtoworlds": poses}
    flags = dict(data_dir=directory, dataset="blender", factor=0, white_bkgd=False, near=float(near), far=float(far), use_pixel_centers=True,
                 config=config, voxel_grid="voxelize", kernel_size=int(kernel_size), kernel_sigma=float(kernel_sigma))
    flags.update(flag_overrides)
    out["flags"] = utils.default_flags(**flags)
    return out
