"""The scenes of tests/test_gpu_table_limits.py (TEST INFRASTRUCTURE, numpy only): the lazy IoR field of a grid with a 2-4 GiB table, the
rays marched through it and the coverage of the table's address range that the oracle's own voxel indices prove.

The field (tests/helpers/lazy_table.py: 1 + 0.5 * clip((a[x] + b[y]) + c[z], 0, 1)):
  * a gentle ramp along every axis (3e-4, 2e-4 and 4.5e-4 per world unit in n: |grad n| = 5.8e-4, below the march's 1e-3 shell threshold;
    4 to 50 ulp of n per voxel), so that the eight corners of EVERY cell hold eight different rows and a lookup from a wrong address cannot
    return the right bits.  The three slopes differ: with equal ones a step in y and a step in z cancel on a grid whose y and z spacings
    nearly agree, and (y0, z1) and (y1, z0) hold the same value;
  * one slab per axis with compact support, SLAB_HEIGHT * max(0, 1 - u^2)^2 at u = (w - SLAB_AT) / SLAB_WIDTH: n rises by 0.1 over a flank
    0.12 wide, |grad n| up to ~1.8 where two slabs cross.  The flanks are the boundary shell — where the gradient bends the rays, so3_mlp
    is evaluated and the backward has pairs.  They hold about 14 % of the nodes: a minority, as in test_gpu_all_backward_kernels.ior_field.
The profiles are evaluated in float64 and rounded once; only their combination is fp32 arithmetic.
"""
from __future__ import annotations

import functools

import numpy as np

from lazy_table import LazyTable
from oracle import ref_np as R

F32 = np.float32
NMIN, NMAX = [-1.5] * 3, [1.5] * 3
NEAR, FAR, N_NODES, N_RAYS = 2.0, 6.0, 192, 96
SHAPES = {"A": (160, 1023, 1024), "B": (300, 510, 1024)}
SLAB_AT, SLAB_WIDTH, SLAB_HEIGHT, RAMP = (0.3, 0.7, -0.5), 0.12, 0.2, (6e-4, 4e-4, 9e-4)


def lazy_field(dims, nmin=NMIN, nmax=NMAX):
    prof = []
    for ax in range(3):
        w = np.linspace(nmin[ax], nmax[ax], dims[ax])
        prof.append((0.1 + RAMP[ax] * (w - nmin[ax]) + SLAB_HEIGHT * np.maximum(0.0, 1.0 - ((w - SLAB_AT[ax]) / SLAB_WIDTH) ** 2) ** 2).astype(F32))
    return LazyTable(*prof, dims, nmin, nmax)


def rays(seed=7):
    """N_RAYS rays from the radius-4 sphere.  The bulk starts above the box's upper-x face and runs ACROSS the x axis towards targets in
    the slice x in [0.9, 1.6] — the upper end of the table's slowest index; the last ones are aimed through the box's corners:
    rays N_RAYS-8 .. N_RAYS-5 leave the box beyond the maximum corner (every index clamps to the LAST entry), rays N_RAYS-4 .. N_RAYS-1
    beyond the minimum corner (entry 0)."""
    rng = np.random.default_rng(seed)
    n = N_RAYS - 8
    tgt = np.stack([rng.uniform(0.9, 1.6, n), rng.uniform(-1.2, 1.6, n), rng.uniform(-1.2, 1.6, n)], -1)
    ox = rng.uniform(1.0, 1.9, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    rad = np.sqrt(16.0 - ox ** 2)
    o = np.stack([ox, rad * np.cos(phi), rad * np.sin(phi)], -1)
    d = tgt - o
    # through a corner, outward: direction mostly along one axis with all three signs those of the corner; the origin lies where that line
    # meets the sphere, 5.1 - 5.5 before the corner (inside the marched [near, far] = [2, 6])
    co, cd = [], []
    for sign in (1.0, -1.0):
        for k in range(4):
            dirn = sign * np.array([[1.0, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, 1.0], [1.0, 0.2, 0.15]][k])
            dirn /= np.linalg.norm(dirn)
            t = sign * np.array([1.51, 1.51, 1.51])
            bq = t @ dirn                                              # |t - s dirn| = 4
            s = bq + np.sqrt(bq * bq - (t @ t - 16.0))
            assert NEAR + 0.5 < s < FAR - 0.3
            co.append(t - s * dirn); cd.append(dirn)
    o = np.concatenate([o, np.array(co)]).astype(F32)
    d = np.concatenate([d, np.array(cd)])
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    assert np.allclose(np.linalg.norm(o, axis=-1), 4.0, atol=1e-5)
    return o, d


def entry_of(x, y, z, dims, layout):
    """int64 position (in 16-byte entries) of voxel (x, y, z) in a table of the given layout (include/rnerf.h: rnerf_table_layout) —
    written out here on its own, not through the package."""
    x, y, z = (np.asarray(v).astype(np.int64) for v in (x, y, z))
    if layout == "reference":
        return (x * dims[1] + y) * dims[2] + z
    by, bz = (dims[1] + 1) // 2, (dims[2] + 1) // 2
    return (((x >> 1) * by + (y >> 1)) * bz + (z >> 1)) * 8 + (x & 1) * 4 + (y & 1) * 2 + (z & 1)


def corner_entries(vox, dims, layout):
    """[..., 8] entries of the eight corners a node gathers, from the oracle's clamped indices vox [..., 6] = x0 x1 y0 y1 z0 z1."""
    return np.stack([entry_of(vox[..., xi], vox[..., yi], vox[..., zi], dims, layout) for xi in (0, 1) for yi in (2, 3) for zi in (4, 5)], -1)


def corner_bytes(vox, dims, layout):
    return 16 * corner_entries(vox, dims, layout)


def last_entry_bytes(dims, layout):
    return int(corner_bytes(np.array([d - 1 for d in dims for _ in (0, 1)]), dims, layout).max())


def coverage(vox, pos, straight, dims, layout):
    """The issue's coverage conditions from the oracle's voxel indices: share of nodes with a corner at or above 2^31 bytes, whether the last
    entry and entry 0 are gathered, and the largest distance of a marched position from its straight ray."""
    cb = corner_bytes(vox, dims, layout)
    return dict(high_share=float((cb.max(-1) >= 2 ** 31).mean()), last=bool((cb == last_entry_bytes(dims, layout)).any()),
                first=bool((cb == 0).any()), bend=float(np.abs(pos - straight).max()))


def distinct_corner_share(lz, vox):
    """Share of the nodes in a proper cell (no index clamped) whose eight corner rows hold eight different n: there a gather from ANY wrong
    corner address changes the interpolated bits."""
    n = np.sort(lz[corner_entries(vox, lz.ndim, "reference")][..., 0], -1)
    proper = (vox[..., 0] < vox[..., 1]) & (vox[..., 2] < vox[..., 3]) & (vox[..., 4] < vox[..., 5])
    return float((np.diff(n, axis=-1) > 0).all(-1)[proper].mean())


@functools.lru_cache(maxsize=None)
def oracle_march(name):
    """R.path_sampler through the lazy table of a big shape, once: (lazy, o, d, outputs with voxel indices, straight-ray positions)."""
    dims = SHAPES[name]
    lz = lazy_field(dims)
    o, d = rays()
    out = R.path_sampler(o, d, lz, list(dims), NMIN, NMAX, NEAR, FAR, N_NODES, return_idx=True)
    step = F32((FAR - NEAR) / (N_NODES - 1))
    straight = o[:, None] + (F32(NEAR) + step * np.arange(N_NODES, dtype=F32))[None, :, None] * d[:, None]
    for a in out:
        a.setflags(write=False)
    return lz, o, d, out, straight
