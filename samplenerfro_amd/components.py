"""Connected components of a voxel grid on the device: the clean-up the reference's README leaves to Blender ("You may remove the noisy
components in the proxy geometry in Blender"), for carved hulls, voxelised proxy meshes and trained densities.

    labels = label(solid, connectivity=6, phase=1)                     # int32 [X,Y,Z] on the device
    roots, sizes, border = stats(labels)                               # ranked: size descending, root ascending
    mask, info = select(solid, keep=1, min_voxels=1, connectivity=6, fill_holes=False)

The label of a voxel of the labelled phase (1: solid, 0: empty) is the smallest linear index x*Y*Z + y*Z + z in its component; every other
voxel is -1.  That is a pure function of the input, so the bytes are the same on every run (rnerf_components_*, csrc/components.hip:
union-find, three launches whatever the grid holds).  The ranking and the keep tables are torch plumbing on the device.
visual_hull.clean, voxelize.clean and extract.extract_mesh(keep=...) are built on `clean_grids`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, current_stream, ptr

CONNECTIVITIES = (6, 18, 26)
COMPLEMENT = {6: 26, 18: 6, 26: 6}          # the digital-topology pairs: the empty phase of a 6-connected solid is 26-connected, and back
DTYPES = {torch.uint8: 0, torch.int32: 1, torch.float32: 2}          # enum rnerf_components_dtype


def _check_selection(keep, min_voxels, connectivity) -> None:
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    if keep is not None and int(keep) < 1:
        raise ValueError(f"keep must be None or >= 1, got {keep!r}")
    if int(min_voxels) < 1:
        raise ValueError(f"min_voxels must be >= 1, got {min_voxels!r}")


def _dims(shape):
    if len(shape) != 3:
        raise ValueError(f"the grid must be [X, Y, Z], got {tuple(shape)}")
    return (C.c_int32 * 3)(*[int(s) for s in shape])


def _solid_uint8(solid, device) -> torch.Tensor:
    """uint8 [X,Y,Z] on the device, non-zero = solid, from a bool / uint8 / any-number grid (torch or numpy); a private copy only if needed."""
    s = solid if isinstance(solid, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(solid))
    if s.ndim != 3:
        raise ValueError(f"the grid must be [X, Y, Z], got {tuple(s.shape)}")
    s = s.detach().to(ops.device_of(s, device=device))
    if s.dtype == torch.bool:
        s = s.to(torch.uint8)
    elif s.dtype != torch.uint8:
        s = (s != 0).to(torch.uint8)
    return s.contiguous()


def label(solid, connectivity: int = 6, phase: int = 1, device=None) -> torch.Tensor:
    """-> labels int32 [X,Y,Z] on the device: the smallest linear index of the voxel's component for voxels of `phase` (1 solid, 0 empty),
    -1 elsewhere.  Raises RnerfError if a kernel reached its iteration cap (a bug, not an input: every loop is bounded by construction)."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    if phase not in (0, 1):
        raise ValueError(f"phase must be 0 (empty) or 1 (solid), got {phase!r}")
    s = _solid_uint8(solid, device)
    lib = _lib.load()
    dims = _dims(s.shape)
    workspace = ops.workspace("rnerf_components_workspace_bytes", C.byref(dims), device=s.device)
    with torch.cuda.device(s.device):
        labels = torch.empty(tuple(s.shape), dtype=torch.int32, device=s.device)
        check(lib.rnerf_components_label(ptr(s), C.byref(dims), int(phase), int(connectivity), ptr(labels), ptr(workspace), current_stream()),
              "rnerf_components_label")
        if int(workspace[:4].view(torch.int32).item()) != 0:          # the error word
            raise _lib.RnerfError("rnerf_components_label: a find / union loop reached its iteration cap")
    return labels


def raw_stats(labels: torch.Tensor):
    """rnerf_components_stats as it is: (size int32 [X,Y,Z], non-zero at root indices; border uint8 [X,Y,Z], 1 at the roots of components
    that touch a face of the grid; counts int64 [2] = components, labelled voxels), all on the device."""
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32 and labels.ndim == 3):
        raise ValueError("labels must be the int32 [X, Y, Z] device tensor of label()")
    labels = labels.contiguous()
    lib = _lib.load()
    dims = _dims(labels.shape)
    with torch.cuda.device(labels.device):
        size = torch.empty(tuple(labels.shape), dtype=torch.int32, device=labels.device)
        border = torch.empty(tuple(labels.shape), dtype=torch.uint8, device=labels.device)
        counts = torch.empty(2, dtype=torch.int64, device=labels.device)
        check(lib.rnerf_components_stats(ptr(labels), C.byref(dims), ptr(size), ptr(border), ptr(counts), current_stream()), "rnerf_components_stats")
    return size, border, counts


def stats(labels: torch.Tensor):
    """-> (roots int32 [K], sizes int64 [K], border bool [K]) on the device, ranked by size descending, ties by the smaller root first
    (one int64 key per root, size * 2^31 - root: a total order)."""
    size, border, _ = raw_stats(labels)
    size = size.reshape(-1)
    roots = torch.nonzero(size, as_tuple=False).reshape(-1)                      # int64, ascending
    sizes = size[roots].to(torch.int64)
    order = torch.argsort(sizes * (1 << 31) - roots, descending=True)          # keys are distinct: the order is total
    roots = roots[order]
    return roots.to(torch.int32), sizes[order], border.reshape(-1)[roots].to(torch.bool)


def apply(grid: torch.Tensor, labels=None, keep=None, drop_value=0, fill_labels=None, fill=None, fill_value=0) -> torch.Tensor:
    """rnerf_components_apply in place on `grid` (uint8 / int32 / float32 [X,Y,Z] on the device): voxels of components whose keep[root] is 0
    become drop_value, voxels of fill_labels' components whose fill[root] is non-zero become fill_value. -> grid."""
    if grid.dtype not in DTYPES or not grid.is_cuda or not grid.is_contiguous():
        raise ValueError("apply: grid must be a contiguous uint8, int32 or float32 device tensor")
    lib = _lib.load()
    dims = _dims(grid.shape)
    with torch.cuda.device(grid.device):
        check(lib.rnerf_components_apply(ptr(labels), ptr(keep), float(drop_value), ptr(fill_labels), ptr(fill), float(fill_value), ptr(grid),
                                         DTYPES[grid.dtype], C.byref(dims), current_stream()), "rnerf_components_apply")
    return grid


def clean_grids(solid: torch.Tensor, payloads, keep: Optional[int] = 1, min_voxels: int = 1, connectivity: int = 6, fill_holes: bool = False) -> dict:
    """The selection of `select` applied in place to `solid` (uint8 [X,Y,Z] on the device, 0 / non-zero; dropped -> 0, filled -> 1) and to
    every (grid, drop_value, fill_value) of `payloads` (same shape; uint8, int32 or float32). -> info."""
    _check_selection(keep, min_voxels, connectivity)
    n = solid.numel()
    labels = label(solid, connectivity, 1)
    roots, sizes, _ = stats(labels)
    K = int(roots.numel())
    kept = sizes >= int(min_voxels)
    if keep is not None:
        kept &= torch.arange(K, device=solid.device) < int(keep)
    n_kept = int(kept.sum().item())
    info = {"components": K, "kept": n_kept, "dropped": K - n_kept, "voxels_dropped": int(sizes[~kept].sum().item()), "voxels_filled": 0,
            "sizes": sizes.cpu().numpy()}
    if n_kept < K:
        table = torch.zeros(n, dtype=torch.uint8, device=solid.device)
        table[roots[kept].long()] = 1
        apply(solid, labels, table, 0)
        for grid, drop_value, _ in payloads:
            apply(grid, labels, table, drop_value)
    if fill_holes:
        del labels
        empty = label(solid, COMPLEMENT[connectivity], 0)
        eroots, esizes, eborder = stats(empty)
        holes = ~eborder
        info["voxels_filled"] = int(esizes[holes].sum().item())
        if info["voxels_filled"]:
            table = torch.zeros(n, dtype=torch.uint8, device=solid.device)
            table[eroots[holes].long()] = 1
            apply(solid, fill_labels=empty, fill=table, fill_value=1)
            for grid, _, fill_value in payloads:
                apply(grid, fill_labels=empty, fill=table, fill_value=fill_value)
    return info


def select(solid, keep: Optional[int] = 1, min_voxels: int = 1, connectivity: int = 6, fill_holes: bool = False, device=None):
    """-> (mask, info).  1. label the solid phase; 2. keep a component iff its rank < keep (None: no rank limit) and its size >= min_voxels;
    3. dropped components become empty; 4. with fill_holes, label the empty phase of the result with the complementary connectivity (26 for
    solid 6, 6 for solid 18 or 26); 5. every empty component without a voxel on a face of the grid becomes solid (a tunnel is no cavity, and
    a cavity that reaches the border stays open).
    mask: on the device, bool for a bool input and uint8 otherwise; kept voxels keep their value, dropped ones are 0, filled ones 1.
    info: components, kept, dropped, voxels_dropped, voxels_filled, sizes (int64 numpy, ranked).
    keep=None, min_voxels=1, fill_holes=False is the identity."""
    _check_selection(keep, min_voxels, connectivity)
    was_bool = (solid.dtype == torch.bool) if isinstance(solid, torch.Tensor) else (np.asarray(solid).dtype == np.bool_)
    s = _solid_uint8(solid, device)
    if isinstance(solid, torch.Tensor) and s.data_ptr() == solid.data_ptr():
        s = s.clone()
    info = clean_grids(s, (), keep, min_voxels, connectivity, fill_holes)
    return (s.to(torch.bool) if was_bool else s), info
