"""Visual-hull carving on the device: the IoR voxel grid of a captured scene from its object masks (calib/make_visual_hull.py:107-146).

    data, ndim, nmin, nmax = from_calib(calib, masks, num_voxels=512, device="cuda:0")     # calib = json.load(open("calib.json"))
    data, ndim, nmin, nmax, count = carve(masks, cam_mat, transforms, 512, return_count=True)
    data, count, info = clean(count, len(transforms), 0.9, keep=1)    # drop the floaters, fill enclosed cavities (components.py)
    save_mesh_pkl(path, count, len(transforms), 0.9, nmin, nmax)      # the dict train.py:209-217 / grid.load_mesh_pkl read
    verts, faces = preview_mesh(count, len(transforms), 0.9, nmin, nmax, out_dir=".")     # mesh_{G}_0_{threshold}.obj

`data` is float32 [G,G,G], x slowest, 1.33 inside the hull and 1.0 outside — the tuple voxelize.voxelize returns, so grid.prepare_grid /
ops.grid_prefilter take it.  The view and projection matrices are formed on the host in numpy float64 as the reference writes them; the
G^3 x V projections, the mask lookups and the counts run on the device (rnerf_visual_hull_count, csrc/hull.hip); preview_mesh is the
hull's marching-cubes mesh the script also exports (:148-157).  Reading image files and calibration are not here.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import Grid, check, current_stream, ptr

CHUNK_BYTES = 1 << 30        # default views_per_chunk: as many mask bytes per upload


def to_view_matrix(mat) -> np.ndarray:
    """calib/make_visual_hull.py:18-28: the world-to-camera matrix of a 4x4 camera-to-world `mat`."""
    mat = np.asarray(mat, np.float64)
    ret = np.eye(4)
    ret[:3, :3] = mat[:3, :3].T
    ret[:3, 3] = (-mat[:3, :3].T @ mat[:3, 3:]).reshape(-1)
    return ret


def init_bounding_box(transforms):
    """create_init_bounding_box (:68-74): a cube of 1.5 x the largest extent of the camera positions around their mean.
    -> (min_point, max_point); the reference returns (max_point, min_point)."""
    poses = np.array(transforms, np.float64)[:, :3, 3]
    pose_avg = np.mean(poses, axis=0)
    max_point = np.max(poses, axis=0)
    min_point = np.min(poses, axis=0)
    side = np.max(max_point - min_point) * 1.5
    return pose_avg - np.ones_like(pose_avg) * side * 0.5, pose_avg + np.ones_like(pose_avg) * side * 0.5


def projection_matrices(cam_mat, transforms) -> np.ndarray:
    """:92-93 and :40: p_mat = [cam_mat | 0], pv = p_mat @ to_view_matrix(T) per view. -> float64 [V, 12] (row-major 3 x 4)."""
    cam_mat = np.array(cam_mat, np.float64)
    if cam_mat.shape != (3, 3):
        raise ValueError(f"cam_mat must be 3 x 3, got {cam_mat.shape}")
    p_mat = np.concatenate([cam_mat, np.zeros((3, 1))], axis=1)
    pv = [p_mat @ to_view_matrix(np.array(t, np.float64)) for t in transforms]
    return np.ascontiguousarray(np.stack(pv).reshape(len(pv), 12))


def _masks_uint8(masks):
    """[V,H,W] uint8 (torch on any device, or numpy) from uint8 / bool arrays or a list of equal-shaped ones; > 0 stays > 0."""
    if isinstance(masks, (list, tuple)):
        if len(masks) == 0:
            raise ValueError("masks: no views")
        tensors = isinstance(masks[0], torch.Tensor)
        masks = [torch.as_tensor(m) if tensors else np.asarray(m) for m in masks]
        shapes = {tuple(m.shape) for m in masks}
        if len(shapes) != 1:
            raise ValueError(f"masks: per-view mask sizes differ ({sorted(shapes)})")
        masks = torch.stack(masks) if tensors else np.stack(masks)
    if isinstance(masks, torch.Tensor):
        if masks.dtype == torch.bool:
            masks = masks.to(torch.uint8)
        if masks.dtype != torch.uint8:
            raise ValueError(f"masks must be uint8 or bool, got {masks.dtype}")
        m = masks.contiguous()
    else:
        m = np.asarray(masks)
        if m.dtype == np.bool_:
            m = m.view(np.uint8)
        if m.dtype != np.uint8:
            raise ValueError(f"masks must be uint8 or bool, got {m.dtype}")
        m = torch.from_numpy(np.ascontiguousarray(m))
    if m.ndim != 3:
        raise ValueError(f"masks must be [V, H, W], got {tuple(m.shape)}")
    return m


def clean(count, num_views: int, threshold: float = 0.9, keep: Optional[int] = 1, min_voxels: int = 1, connectivity: int = 6,
          fill_holes: bool = True, ior_inside: float = 1.33, ior_outside: float = 1.0):
    """The hull without its floaters: what the reference's README leaves to Blender before voxelising ("remove the noisy components in the
    proxy geometry").  The clamped projections (:129-130) let voxels far outside every frustum vote with the masks' edges, so a carved
    grid regularly holds loose parts beside the object.  -> (data float32 [G,G,G], count_clean int32 [G,G,G], info) on count's device.
    Solid is count / num_views > threshold in float64, as preview_mesh and save_mesh_pkl evaluate it; components.select's rules (keep the
    `keep` largest components of at least min_voxels voxels; with fill_holes, enclosed cavities become solid).  count_clean is count on
    kept voxels, 0 on dropped ones and num_views on filled ones, so save_mesh_pkl(path, count_clean, ...) and preview_mesh(count_clean, ...)
    agree with `data`.  keep=None, min_voxels=1, fill_holes=False changes nothing."""
    from . import components
    components._check_selection(keep, min_voxels, connectivity)
    if int(num_views) < 1:
        raise ValueError("clean: num_views must be >= 1")
    if not 0.0 <= float(threshold):
        raise ValueError("clean: threshold must be >= 0 (a dropped voxel, count 0, has to fail count / num_views > threshold)")
    if fill_holes and float(threshold) >= 1.0:
        raise ValueError("clean: fill_holes needs threshold < 1 (a filled voxel, count = num_views, has to pass count / num_views > threshold)")
    c = count if isinstance(count, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(count))
    if c.ndim != 3:
        raise ValueError(f"count must be [X, Y, Z], got {tuple(c.shape)}")
    if not c.is_cuda:
        c = c.to(torch.device("cuda", torch.cuda.current_device()))
    count_clean = c.detach().to(torch.int32).clone().contiguous()
    solid = (count_clean.to(torch.float64) / num_views > threshold).to(torch.uint8)
    info = components.clean_grids(solid, [(count_clean, 0, int(num_views))], keep, min_voxels, connectivity, fill_holes)
    inside = count_clean.to(torch.float64) / num_views > threshold
    data = torch.where(inside, torch.tensor(float(ior_inside), dtype=torch.float64, device=c.device),
                       torch.tensor(float(ior_outside), dtype=torch.float64, device=c.device)).to(torch.float32)
    return data, count_clean, info


_clean = clean          # carve's keyword of the same name hides the function


def carve(masks, cam_mat, transforms, num_voxels: int, min_point=None, max_point=None, threshold: float = 0.9, device=None,
          views_per_chunk: Optional[int] = None, return_count: bool = False, ior_inside: float = 1.33, ior_outside: float = 1.0,
          clean: Optional[dict] = None):
    """calib/make_visual_hull.py:107-141. -> (data float32 [G,G,G] on `device`, ndim, nmin, nmax[, count int32 [G,G,G]]).
    masks: [V,H,W] uint8 or bool (torch or numpy) or a list of [H,W] arrays, > 0 = object; transforms: V camera-to-world 4x4 matrices;
    min_point / max_point None: the default box of init_bounding_box.  The views go to the device views_per_chunk at a time.
    clean: None, or the keywords of clean() (keep, min_voxels, connectivity, fill_holes) as a dict: data and count are then the cleaned ones."""
    m = _masks_uint8(masks)
    V, H, W = (int(s) for s in m.shape)
    if len(transforms) != V:
        raise ValueError(f"{V} masks but {len(transforms)} transforms")
    pv = projection_matrices(cam_mat, transforms)
    if min_point is None or max_point is None:
        min_point, max_point = init_bounding_box(transforms)
    nmin, nmax = [float(v) for v in min_point], [float(v) for v in max_point]
    G = int(num_voxels)
    lib = _lib.load()
    device = ops.device_of(device=device)
    spec = Grid.make([G] * 3, nmin, nmax)
    chunk = int(views_per_chunk) if views_per_chunk else max(1, CHUNK_BYTES // (H * W))
    chunk = max(1, min(chunk, V))
    workspace = ops.workspace("rnerf_visual_hull_workspace_bytes", chunk, H, W, device=device)
    with torch.cuda.device(device):
        count = torch.empty((G, G, G), dtype=torch.int32, device=device)
        out = torch.empty((G, G, G), dtype=torch.float32, device=device)
        for v0 in range(0, V, chunk):
            n = min(chunk, V - v0)
            m_d = m[v0:v0 + n].to(device)                            # (named: the blocks must outlive the launch)
            pv_d = torch.from_numpy(pv[v0:v0 + n]).to(device)
            check(lib.rnerf_visual_hull_count(ptr(m_d), n, H, W, ptr(pv_d), C.byref(spec), 1 if v0 else 0, ptr(count), ptr(workspace),
                                              current_stream()), "rnerf_visual_hull_count")
        check(lib.rnerf_visual_hull_finalize(ptr(count), C.byref(spec), V, float(threshold), float(ior_inside), float(ior_outside), ptr(out),
                                             current_stream()), "rnerf_visual_hull_finalize")
        if clean is not None:
            out, count, _ = _clean(count, V, threshold, ior_inside=ior_inside, ior_outside=ior_outside, **clean)
    ret = (out, [G] * 3, nmin, nmax)
    return ret + (count,) if return_count else ret


def from_calib(calib: dict, masks, num_voxels: int, **kwargs):
    """carve() from the dict of the reference's calib.json: "cam_mat" and "frames"[i]["transform_matrix"] (:77-78,92-103); masks in the
    order of the frames."""
    return carve(masks, calib["cam_mat"], [f["transform_matrix"] for f in calib["frames"]], num_voxels, **kwargs)


def save_mesh_pkl(path: str, count, num_views: int, threshold: float, min_point, max_point) -> None:
    """The dict of :139-146.  "data" is formed on the host in float64 from the counts with the reference's expressions (:136,141), so it
    equals the reference's array bit for bit (1.33 there is 0.33 + 1.0 in float64, not a float32 widened)."""
    c = count.detach().cpu().numpy() if isinstance(count, torch.Tensor) else np.asarray(count)
    if c.ndim != 3 or not (c.shape[0] == c.shape[1] == c.shape[2]):
        raise ValueError(f"count must be [G, G, G], got {c.shape}")
    frac = c.astype(np.float64)
    frac /= num_views
    with open(path, "wb") as f:
        pickle.dump({"data": (frac > threshold).reshape(-1, 1) * 0.33 + 1.0, "extent": 0, "min_point": np.asarray(min_point, np.float64),
                     "max_point": np.asarray(max_point, np.float64), "num_voxels": int(c.shape[0])}, f)


def preview_coords(verts, num_voxels: int, min_point, max_point):
    """:151-154: marching-cubes vertices (index units) / num_voxels, scaled into the box.  (The voxel centres divide by num_voxels - 1,
    :112-120; the script's mesh is smaller than the grid by that factor, and so is this one.)"""
    lo = np.asarray(min_point, np.float64); span = np.asarray(max_point, np.float64) - lo
    den = np.full(3, float(num_voxels))
    if isinstance(verts, torch.Tensor):            # the divisor as a tensor: torch multiplies by the reciprocal of a Python scalar
        lo, span, den = (torch.from_numpy(a).to(verts.device) for a in (lo, span, den))
    return verts / den * span + lo


def preview_mesh(count, num_views: int, threshold: float, min_point, max_point, out_dir: Optional[str] = None, device=None):
    """calib/make_visual_hull.py:148-157: marching cubes of the boolean grid count / num_views > threshold (float64, as :136) at iso 0.5,
    vertices in the script's own transform (preview_coords). -> (verts float64 [V,3], faces int32 [F,3]) on the device; with out_dir the
    OBJ is written there as mesh_{G}_0_{threshold}.obj.  Every vertex sits half way along a grid edge.  The mesh is marching_cubes.py's,
    not PyMCubes' vertex for vertex."""
    from . import marching_cubes as mc
    c = count if isinstance(count, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(count))
    if c.ndim != 3 or not (c.shape[0] == c.shape[1] == c.shape[2]):
        raise ValueError(f"count must be [G, G, G], got {tuple(c.shape)}")
    G = int(c.shape[0])
    if device is not None:
        c = c.to(device)
    elif not c.is_cuda:
        c = c.to(torch.device("cuda", torch.cuda.current_device()))
    verts, faces = mc.marching_cubes(c.to(torch.float64) / num_views > threshold, 0.5)
    verts = preview_coords(verts, G, min_point, max_point)
    if out_dir is not None:
        mc.save_obj(os.path.join(out_dir, f"mesh_{G}_0_{threshold}.obj"), verts, faces)
    return verts, faces
