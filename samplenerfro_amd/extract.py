"""A trained field's density as a mesh (extract_mesh.py:232-268): the lattice query and marching cubes, both on the device.

    verts, faces = extract_mesh(model, variables, resolution=256, range=1.2, threshold=0.1)     # world units
    marching_cubes.save_obj(path, verts, faces)

Deviation from the reference, whose code for this sits after an exit() (:226) and never ran: it builds the lattice with np.meshgrid's
default "xy" indexing, which swaps x and y between the query points and the array the mesh is taken from, and exports vertices / N - 0.5,
which is the unit cube whatever --range is.  Here the lattice is indexed "ij" (array axis = world axis) and the mesh comes back in world
units: index i of an axis is i / N * 2 range - range.
"""
from __future__ import annotations

import numpy as np
import torch

from . import marching_cubes as mc

_range = range          # the reference's flag name `range` is the parameter name below


def alpha_grid(model, variables, resolution: int = 256, range: float = 1.2, chunk: int = 1 << 18, device=None) -> torch.Tensor:
    """extract_mesh.py:232-245: NerfModel.sample_points' alpha with zero view directions over the (N + 1)^3 lattice
    linspace(-range, range, N + 1)^3 (float32, "ij"), `chunk` points per call. -> float32 [N+1, N+1, N+1] on the device."""
    N = int(resolution)
    if N < 1 or chunk < 1:
        raise ValueError("alpha_grid: resolution and chunk must be >= 1")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    t = torch.from_numpy(np.linspace(-range, range, N + 1).astype(np.float32)).to(device)
    flat = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 1, 3)
    out = torch.empty(flat.shape[0], dtype=torch.float32, device=device)
    for i in _range(0, flat.shape[0], int(chunk)):
        pts = flat[i:i + chunk].contiguous()
        out[i:i + chunk] = model.apply(variables, pts, torch.zeros_like(pts), method=model.sample_points)[1].reshape(-1)
    return out.reshape(N + 1, N + 1, N + 1)


def extract_mesh(model, variables, resolution: int = 256, range: float = 1.2, threshold: float = 0.1, chunk: int = 1 << 18, device=None,
                 keep=None, min_voxels: int = 1, connectivity: int = 6):
    """extract_mesh.py:232-268 (flags :40-42): alpha_grid -> marching cubes at `threshold` -> world coordinates.
    -> (verts float64 [V,3] within [-range, range]^3, faces int32 [F,3]) on the device.
    keep / min_voxels / connectivity: components.select's rules on alpha > threshold (float64, marching cubes' own test); the alpha of
    dropped samples is 0 before marching cubes, so the floaters of the density leave no crumbs.  keep=None, min_voxels=1: nothing is done."""
    from . import components
    components._check_selection(keep, min_voxels, connectivity)
    grid = alpha_grid(model, variables, resolution, range, chunk, device)
    if keep is not None or int(min_voxels) > 1:
        grid = grid.detach().to(torch.float32).clone().contiguous()
        solid = (grid.to(torch.float64) > float(threshold)).to(torch.uint8)
        components.clean_grids(solid, [(grid, 0.0, 0.0)], keep, min_voxels, connectivity, False)
    verts, faces = mc.marching_cubes(grid, threshold)
    den = torch.full((3,), float(int(resolution)), dtype=torch.float64, device=verts.device)      # a tensor: a true division
    return verts / den * (2.0 * range) - range, faces
