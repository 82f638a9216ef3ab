"""A lazily evaluated IoR table for grids too large to build on the host (TEST INFRASTRUCTURE, no device needed).

R.build_table of a 2.5 GiB table costs seconds and ~10 GB of temporaries; the float64 references would want another copy.  The oracle's
consumers (R.linear3, R.path_sampler, TR.linear3_t and tests/helpers/all_backward_ref.py) read the table only as `table[flat_index_array]`,
so a table that computes exactly the requested rows serves them unchanged.

The grid is a function of three 1-D float32 profiles a, b, c,

    n(x, y, z) = offset + scale * clip((a[x] + b[y]) + c[z], 0, 1)

made of individually rounded fp32 adds, one multiply and a clip.  numpy on the host and torch on the device (eager ops, nothing fused or
contracted) therefore produce the same bits, and no 3-D array ever exists on the host.  A row is (n, dn/dx, dn/dy, dn/dz) exactly as
R.build_table forms it: central differences over the edge-padded grid (np.pad(..., "edge")), divided through R._cdiv by 2 * ndelta.
"""
from __future__ import annotations

import numpy as np

from oracle import ref_np as R

F32 = np.float32


class LazyTable:
    """The numpy face: `table[flat]` -> float32 rows [..., 4] at reference-order flat indices x * Gy * Gz + y * Gz + z."""

    def __init__(self, a, b, c, ndim, nmin, nmax, offset=1.0, scale=0.5):
        self.prof = [np.ascontiguousarray(p, F32) for p in (a, b, c)]
        self.ndim = [int(v) for v in ndim]
        assert [p.shape for p in self.prof] == [(n,) for n in self.ndim] and min(self.ndim) >= 2
        self.nmin, self.nmax = [float(v) for v in nmin], [float(v) for v in nmax]
        self.offset, self.scale = F32(offset), F32(scale)
        self.shape = (self.ndim[0] * self.ndim[1] * self.ndim[2], 4)

    def value(self, x, y, z):
        """n at integer voxel coordinates (arrays of one shape), in the rounding order of the module docstring."""
        a, b, c = self.prof
        s = np.clip((a[x] + b[y]) + c[z], F32(0), F32(1))
        return self.offset + self.scale * s

    def __getitem__(self, flat):
        flat = np.asarray(flat).astype(np.int64)
        assert flat.size == 0 or (int(flat.min()) >= 0 and int(flat.max()) < self.shape[0])
        dx, dy, dz = self.ndim
        i = [flat // (dy * dz), (flat // dz) % dy, flat % dz]
        ndelta = R.compute_ndelta(self.ndim, self.nmin, self.nmax)
        cols = [self.value(*i)]
        for ax in range(3):                                   # np.pad(g, 1, "edge"): p[k + 2] - p[k] = g[min(k + 1, G - 1)] - g[max(k - 1, 0)]
            hi, lo = list(i), list(i)
            hi[ax] = np.minimum(i[ax] + 1, self.ndim[ax] - 1)
            lo[ax] = np.maximum(i[ax] - 1, 0)
            cols.append(R._cdiv(self.value(*hi) - self.value(*lo), 2 * ndelta[ax], F32))
        return np.stack(cols, axis=-1).astype(F32)

    def dense_grid(self):
        """The whole grid as a host array [Gx, Gy, Gz] (small grids only: what R.build_table is fed in the host test)."""
        x, y, z = np.meshgrid(*[np.arange(n) for n in self.ndim], indexing="ij")
        return self.value(x, y, z)

    def device_grid(self, device):
        """The same grid built by torch broadcasting on `device`: one [Gx, Gy, Gz] float32 tensor, every op in place after the first sum."""
        import torch
        a, b, c = (torch.from_numpy(p).to(device) for p in self.prof)
        s = (a[:, None, None] + b[None, :, None]) + c[None, None, :]
        s.clamp_(0.0, 1.0).mul_(float(self.scale)).add_(float(self.offset))
        return s

    def torch_face(self, dtype=None):
        import torch
        return LazyTorchTable(self, torch.float64 if dtype is None else dtype)


class LazyTorchTable:
    """The torch face: the same fp32 rows as float64 (what `table.detach().cpu().double()` of the device table gives the float64
    references); `.float()` is the float32 copy their noise-floor twins are fed."""

    def __init__(self, lazy, dtype):
        self.lazy, self.dtype, self.shape = lazy, dtype, lazy.shape

    def __getitem__(self, flat):
        import torch
        return torch.from_numpy(self.lazy[flat.detach().cpu().numpy()]).to(self.dtype)

    def float(self):
        import torch
        return LazyTorchTable(self.lazy, torch.float32)

    def double(self):
        import torch
        return LazyTorchTable(self.lazy, torch.float64)
