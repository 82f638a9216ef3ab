"""Marching cubes on the device: the mesh of an iso-surface of a grid that voxelize / visual_hull.carve / extract.alpha_grid left there.

    verts, faces = marching_cubes(field, iso)            # float64 [V,3] in index units (sample i at coordinate i), int32 [F,3]
    save_obj(path, verts / N - 0.5, faces)               # the OBJ voxelize_mesh.py:133-135 exports

Stands in for mcubes.marching_cubes at voxelize_mesh.py:126, calib/make_visual_hull.py:148 and extract_mesh.py:259 (rnerf_marching_cubes_*,
csrc/mcubes.hip).  A sample is solid iff float64(f) > iso; vertices are ordered by grid edge, triangles by cell, counter-clockwise seen
from the empty side, and the surface of any field is closed except where it leaves the grid (include/rnerf.h).  PyMCubes' own tie rule,
vertex order and triangulation of each case are not reproduced.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, current_stream, ptr


def marching_cubes(field, iso: float, device=None):
    """-> (verts float64 [V,3] on the device in index units, faces int32 [F,3]).  field: [Gx,Gy,Gz] torch or numpy; bool, uint8 and float64
    are converted to float32.  One 16-byte readback (the totals) between the counting and the emitting call."""
    lib = _lib.load()
    f = field if isinstance(field, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(field))
    if f.ndim != 3:
        raise ValueError(f"field must be [Gx, Gy, Gz], got {tuple(f.shape)}")
    device = ops.device_of(f, device=device)
    f = f.detach().to(device=device, dtype=torch.float32).contiguous()
    dims = (C.c_int32 * 3)(*[int(s) for s in f.shape])
    workspace = ops.workspace("rnerf_marching_cubes_workspace_bytes", C.byref(dims), device=device)
    with torch.cuda.device(device):
        totals = torch.empty(2, dtype=torch.int64, device=device)
        check(lib.rnerf_marching_cubes_count(ptr(f), C.byref(dims), float(iso), ptr(workspace), ptr(totals), current_stream()),
              "rnerf_marching_cubes_count")
        V, F = (int(v) for v in totals.cpu())
        verts = torch.empty((V, 3), dtype=torch.float64, device=device)
        faces = torch.empty((F, 3), dtype=torch.int32, device=device)
        overflow = torch.empty(1, dtype=torch.int32, device=device)
        check(lib.rnerf_marching_cubes_emit(ptr(f), C.byref(dims), float(iso), ptr(workspace), ptr(verts) if V else None, V,
                                            ptr(faces) if F else None, F, ptr(overflow), current_stream()), "rnerf_marching_cubes_emit")
    return verts, faces


def case_table() -> np.ndarray:
    """The case table the kernels use: int8 [256, 16], up to five triangles of three edge ids per case, -1 padded (no device needed)."""
    out = np.empty((256, 16), np.int8)
    check(_lib.load().rnerf_marching_cubes_table(out.ctypes.data), "rnerf_marching_cubes_table")
    return out


def save_obj(path: str, verts, faces) -> None:
    """Wavefront OBJ with `v` and 1-based `f` records; %.17g, so voxelize.load_obj returns the same float64 bits."""
    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    v = v.astype(np.float64).reshape(-1, 3); f = f.astype(np.int64).reshape(-1, 3) + 1
    with open(path, "w") as out:
        out.write("".join("v %.17g %.17g %.17g\n" % (a, b, c) for a, b, c in v.tolist()))
        out.write("".join("f %d %d %d\n" % (a, b, c) for a, b, c in f.tolist()))
