"""Object masks for masked / cropped evaluation: the silhouette of a mesh from a test camera, dilated (metric/render_mask.py:84-94).

    masks = list(render_masks(verts, faces, camtoworlds, H, W, focal=focal))          # uint8 [H, W] on the device, 0 / 255
    res = evaluate.evaluate(model, variables, views, rng, masks=masks, mask_mode="mask")
    save_mask(os.path.join(data_dir, mask_file_name(frame["file_path"], "blender")), masks[0])

The reference draws the mesh with pyrender (an OpenGL context), takes `depth != 0` (:91) and dilates with a 35 x 35 box (:92-93); its
scorers (metric/summary.py:177-205, metric/compare.py:167-197) multiply both images by the mask and / or cut them to its bounding
rectangle.  Here the mesh is rasterised on the device with the camera model of ops.generate_rays (rnerf_mesh_depth, csrc/raster.hip;
include/rnerf.h holds the fill rule) and dilated there (rnerf_mask_dilate).  verts / faces are what voxelize.load_obj,
marching_cubes.marching_cubes or the preview_mesh functions return, in WORLD coordinates.

A mask is rendered with the view's own intrinsics at the resolution the view is evaluated at, so the `HALF` resizing and central crop
of the reference's scorers (summary.py:183-194), which bring a full-size mask file down to the evaluated size, have nothing to do here.
pyrender's shaded colour image, clipping against the near plane and the error-map images of the scorers are not here.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import RnerfError, check, current_stream, ptr


def upload_mesh(verts, faces, device=None):
    """-> (verts float64 [V, 3], faces int32 [F, 3]) contiguous on the device; the face indices are checked here (the kernels trust them)."""
    device = ops.device_of(verts, faces, device=device)
    v = verts if isinstance(verts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(verts, np.float64)))
    f = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(faces).astype(np.int32, copy=False)))
    v = v.detach().to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()
    f = f.detach().to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()
    if f.numel():
        lo, hi = int(f.min()), int(f.max())
        if lo < 0 or hi >= v.shape[0]:
            raise ValueError(f"faces index vertices {lo} .. {hi}, the mesh has {v.shape[0]}")
    return v, f


def _camera(H: int, W: int, focal, cam_mat, pixel_center: bool):
    """The camera arguments of ops.generate_rays: Blender model with `focal`, OpenCV model with `cam_mat`."""
    if (focal is None) == (cam_mat is None):
        raise ValueError("give focal (Blender model) or cam_mat (OpenCV model)")
    return ops.camera_args(H, W, focal, cam_mat) + (0.5 if pixel_center else 0.0,)


def _render_uploaded(v, f, camtoworld, H, W, cam, znear, zfar, want_tri, want_hits, allow_skipped, workspace=None):
    lib = _lib.load()
    dev = v.device
    if isinstance(camtoworld, torch.Tensor):
        camtoworld = camtoworld.detach().cpu().numpy()
    c2w = np.ascontiguousarray(np.asarray(camtoworld, np.float32)[:3, :4])
    V, F = int(v.shape[0]), int(f.shape[0])
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = ops.workspace("rnerf_mesh_depth_workspace_bytes", V, F, int(H), int(W), device=dev)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        tri = torch.empty((H, W), dtype=torch.int32, device=dev) if want_tri else None
        hits = torch.empty((H, W), dtype=torch.int32, device=dev) if want_hits else None
        skipped = torch.empty(1, dtype=torch.int64, device=dev)
        check(lib.rnerf_mesh_depth(ptr(v) if V else None, V, ptr(f) if F else None, F, c2w.ctypes.data_as(C.c_void_p), cam[0], cam[1], cam[2],
                                   cam[3], cam[4], cam[5], int(H), int(W), float(znear), float(zfar), ptr(depth), ptr(tri), ptr(hits),
                                   ptr(skipped), ptr(workspace) if F else None, current_stream()), "rnerf_mesh_depth")
        if not allow_skipped:
            n = int(skipped.cpu())
            if n:
                raise RnerfError(f"render_depth: {n} of {F} triangles have a vertex at or behind the camera plane and were not drawn "
                                 "(there is no clipping; allow_skipped=True accepts that)")
    return depth, tri, hits, skipped


def render_depth(verts, faces, camtoworld, H: int, W: int, *, focal: Optional[float] = None, cam_mat=None, pixel_center: bool = True,
                 znear: float = 0.1, zfar: float = 100.0, device=None, return_tri: bool = False, return_hits: bool = False,
                 allow_skipped: bool = False):
    """First-surface depth of the mesh from one view (rnerf_mesh_depth): float32 [H, W] on the device, the distance along the view axis
    (pyrender's depth buffer, Blender's Z pass), 0 where no triangle is hit between znear and zfar.  verts [V, 3] / faces [F, 3]: numpy
    arrays or device tensors; camtoworld, focal / cam_mat, pixel_center: as ops.generate_rays.  return_tri / return_hits append the
    int32 [H, W] index of the first triangle (-1: none) / number of triangles each pixel's ray passes through.  Raises RnerfError when
    triangles reach behind the camera plane (they are not drawn) unless allow_skipped."""
    v, f = upload_mesh(verts, faces, device)
    depth, tri, hits, _ = _render_uploaded(v, f, camtoworld, int(H), int(W), _camera(H, W, focal, cam_mat, pixel_center), znear, zfar,
                                           return_tri, return_hits, allow_skipped)
    out = (depth,) + ((tri,) if return_tri else ()) + ((hits,) if return_hits else ())
    return out if len(out) > 1 else depth


def _dilate(mask: torch.Tensor, ky: int, kx: int, want_bbox: bool):
    lib = _lib.load()
    if mask.ndim != 2 or mask.dtype != torch.uint8 or not mask.is_cuda:
        raise ValueError("mask must be a uint8 [H, W] device tensor")
    m = mask.contiguous()
    H, W = int(m.shape[0]), int(m.shape[1])
    workspace = ops.workspace("rnerf_mask_dilate_workspace_bytes", H, W, device=m.device)
    with torch.cuda.device(m.device):
        out = torch.empty_like(m)
        bbox = torch.empty(4, dtype=torch.int32, device=m.device) if want_bbox else None
        check(lib.rnerf_mask_dilate(ptr(m), H, W, int(ky), int(kx), ptr(out), ptr(bbox), ptr(workspace), current_stream()), "rnerf_mask_dilate")
    return out, bbox


def _as_mask(mask, device=None) -> torch.Tensor:
    """uint8 [H, W] on the device, 1 where `mask` > 0 (bool, 0 / 1 and 0 / 255 masks, float or integer, numpy or torch)."""
    m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
    if m.ndim == 3 and m.shape[-1] == 1:
        m = m[..., 0]
    if m.ndim != 2:
        raise ValueError(f"a mask must be [H, W], got {tuple(m.shape)}")
    return (m.to(ops.device_of(m, device=device)) > 0).to(torch.uint8)


def dilate(mask, size=35) -> torch.Tensor:
    """cv2.dilate(mask, np.ones((size, size)), iterations=1) (render_mask.py:92-93) on the device: uint8 [H, W], 255 where any pixel of the
    box centred on the pixel is > 0.  size: an odd int or (ky, kx)."""
    ky, kx = (size, size) if np.isscalar(size) else size
    return _dilate(_as_mask(mask), ky, kx, False)[0]


def bounding_rect(mask):
    """cv2.boundingRect(mask) (summary.py:202): (x, y, w, h) Python ints of the pixels > 0; (0, 0, 0, 0) for an empty mask."""
    _, bbox = _dilate(_as_mask(mask), 1, 1, True)
    return tuple(int(v) for v in bbox.cpu())


def render_masks(verts, faces, camtoworlds: Iterable, H: int, W: int, *, dilate: int = 35, focal: Optional[float] = None, cam_mat=None,
                 pixel_center: bool = True, znear: float = 0.1, zfar: float = 100.0, device=None, allow_skipped: bool = False):
    """render_mask.py for every view: yields one uint8 [H, W] device tensor (0 / 255) per camera-to-world matrix.  The mesh is uploaded
    once and the workspace is shared.  dilate: the box size (35 there; 0 or 1: the bare silhouette)."""
    v, f = upload_mesh(verts, faces, device)
    cam = _camera(H, W, focal, cam_mat, pixel_center)
    workspace = ops.workspace("rnerf_mesh_depth_workspace_bytes", int(v.shape[0]), int(f.shape[0]), int(H), int(W), device=v.device)
    for c2w in camtoworlds:
        depth, _, _, _ = _render_uploaded(v, f, c2w, int(H), int(W), cam, znear, zfar, False, False, allow_skipped, workspace)
        mask = (depth != 0).to(torch.uint8)                                   # render_mask.py:91
        yield _dilate(mask, int(dilate), int(dilate), False)[0] if dilate and int(dilate) > 1 else mask * 255


def render_mask(verts, faces, camtoworld, H: int, W: int, **kwargs) -> torch.Tensor:
    """render_mask.py:84-93 for one view: uint8 [H, W] holding 0 / 255 (keywords as render_masks)."""
    return next(iter(render_masks(verts, faces, [camtoworld], H, W, **kwargs)))


def save_mask(path: str, mask) -> None:
    """The single-channel 8-bit PNG cv2.imwrite writes at render_mask.py:94 (0 / 255)."""
    from PIL import Image
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    Image.fromarray(((m > 0) * 255).astype(np.uint8), mode="L").save(path, "PNG")


def mask_file_name(file_path: str, dataset: str = "blender") -> str:
    """render_mask.py:88-89, relative to the scene's directory: the frame's directory joined with mask_<name>.png, where <name> is the
    last component of the frame's file_path ("blender": as it is, it carries no extension there; "opencv": without its 4-character
    extension).  summary.py:136,143 reads the same paths back."""
    if dataset not in ("blender", "opencv"):
        raise ValueError(f"dataset must be 'blender' or 'opencv', got {dataset!r}")
    directory, fname = os.path.split(file_path)
    return os.path.join(directory, "mask_" + (fname if dataset == "blender" else fname[:-4]) + ".png")
