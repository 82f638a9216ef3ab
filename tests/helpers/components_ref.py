"""Canonical connected-component labels in pure numpy, independent of samplenerfro_amd/components.py.

The label of a voxel of the labelled phase is the smallest linear index (x*Y*Z + y*Z + z) in its component, -1 elsewhere.  Over the list
of adjacent same-phase pairs: hook parent[max] <- min (np.minimum.at), then pointer-jump to a fixed point, repeated until nothing changes.
select / fill_holes on top of it with the rules of components.select.
"""
import itertools

import numpy as np

COMPLEMENT = {6: 26, 18: 6, 26: 6}


def offsets(connectivity):
    """Half of the neighbourhood (each pair once): the offsets that are lexicographically positive."""
    top = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0) and sum(c != 0 for c in o) <= top]


def _pairs(on, connectivity):
    X, Y, Z = on.shape
    idx = np.arange(on.size, dtype=np.int64).reshape(on.shape)
    a_all, b_all = [], []
    for dx, dy, dz in offsets(connectivity):
        sa = tuple(slice(max(0, -d), n - max(0, d)) for d, n in ((dx, X), (dy, Y), (dz, Z)))
        sb = tuple(slice(max(0, d), n - max(0, -d)) for d, n in ((dx, X), (dy, Y), (dz, Z)))
        both = on[sa] & on[sb]
        a_all.append(idx[sa][both]); b_all.append(idx[sb][both])
    return np.concatenate(a_all), np.concatenate(b_all)


def label(solid, connectivity=6, phase=1):
    """-> int32 [X,Y,Z]."""
    on = (np.asarray(solid) != 0) == bool(phase)
    a, b = _pairs(on, connectivity)
    parent = np.arange(on.size, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            break
        hi, lo = np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ]
        np.minimum.at(parent, hi, lo)
        while True:
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped
    out = np.where(on.reshape(-1), parent, -1).astype(np.int32)
    return out.reshape(on.shape)


def stats(labels):
    """-> (roots, sizes, border) ranked by size descending, then root ascending."""
    flat = labels.reshape(-1)
    sizes_all = np.bincount(flat[flat >= 0], minlength=flat.size)
    roots = np.nonzero(sizes_all)[0]
    face = np.zeros(labels.shape, bool)
    for ax in range(3):
        sl = [slice(None)] * 3
        sl[ax] = 0; face[tuple(sl)] = True
        sl[ax] = -1; face[tuple(sl)] = True
    touches = np.zeros(flat.size, bool)
    touches[flat[(flat >= 0) & face.reshape(-1)]] = True
    order = np.lexsort((roots, -sizes_all[roots]))
    roots = roots[order]
    return roots.astype(np.int32), sizes_all[roots].astype(np.int64), touches[roots]


def select(solid, keep=1, min_voxels=1, connectivity=6, fill_holes=False):
    """-> (mask bool [X,Y,Z], dropped bool, filled bool)."""
    on = np.asarray(solid) != 0
    lab = label(on, connectivity, 1)
    roots, sizes, _ = stats(lab)
    ok = sizes >= min_voxels
    if keep is not None:
        ok &= np.arange(len(roots)) < keep
    mask = on & np.isin(lab, roots[ok])
    dropped = on & ~mask
    filled = np.zeros_like(on)
    if fill_holes:
        elab = label(mask, COMPLEMENT[connectivity], 0)
        eroots, _, eborder = stats(elab)
        filled = np.isin(elab, eroots[~eborder])
        mask = mask | filled
    return mask, dropped, filled
