"""numpy restatement of rnerf/vis.py as include/rnerf.h specifies rnerf_vis_depth / rnerf_vis_normals, in a chosen dtype
(float64: the arbiter; float32: the floor of the float32 rule).  No scipy, no matplotlib: the convolution is written out and the turbo
list is read from the committed csrc/turbo_table.h (tests/test_vis_host.py checks both against the libraries).

Orders that the formulas leave open are fixed here as the header fixes them: the convolution adds its nine products in kernel order
from 0, the running sum of acc' is sequential in the sorted order."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EPS = float(np.finfo(np.float32).eps)          # 2^-23, whatever the dtype
CURVES = ("neg_log", "identity", "reciprocal", "log")


def turbo_table(dtype=np.float64):
    """The 256 x 3 list of csrc/turbo_table.h (its decimals are matplotlib's doubles)."""
    text = open(os.path.join(ROOT, "samplenerfro_amd", "csrc", "turbo_table.h")).read()
    body = text[text.index("RNERF_TURBO_TABLE {"):]
    vals = [float(v) for v in re.findall(r"([0-9.eE+-]+)f", body)]
    return np.array(vals, np.float64).reshape(256, 3).astype(dtype)


def sinebow(h, dtype=np.float64):
    h = np.asarray(h, dtype)
    f = lambda x: np.sin(dtype(np.pi) * x) ** 2
    return np.stack([f(dtype(3 / 6) - h), f(dtype(5 / 6) - h), f(dtype(7 / 6) - h)], -1)


def convolve2d_same(z, k, dtype=np.float64):
    """scipy.signal.convolve2d(z, k, mode='same') for a 3 x 3 k: out[r][c] = sum over (p, q) of k[p][q] z[r + 1 - p][c + 1 - q], zero
    outside, the nine products added in kernel order from 0 (0 * NaN = NaN: every tap counts)."""
    z, k = np.asarray(z, dtype), np.asarray(k, dtype)
    H, W = z.shape
    pad = np.zeros((H + 2, W + 2), dtype)
    pad[1:-1, 1:-1] = z
    out = np.zeros((H, W), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(3):
            for q in range(3):
                out = out + k[p, q] * pad[2 - p:2 - p + H, 2 - q:2 - q + W]
    return out


def normal_kernels(dtype=np.float64):
    blur, edge = np.array([1, 2, 1], dtype) / dtype(4), np.array([-1, 0, 1], dtype) / dtype(2)
    return blur[None, :] * edge[:, None], blur[:, None] * edge[None, :]          # dy's, dx's (vis.py:38-39)


def depth_to_normals(depth, dtype=np.float64):
    ky, kx = normal_kernels(dtype)
    dy, dx = convolve2d_same(depth, ky, dtype), convolve2d_same(depth, kx, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        inv = dtype(1) / np.sqrt((dtype(1) + dx * dx) + dy * dy)
        return np.stack([dx * inv, dy * inv, inv], -1)


def normals_scaling(depth, dtype=np.float64):
    depth = np.asarray(depth, dtype)
    mask = ~np.isnan(depth)
    x, y = np.meshgrid(np.arange(depth.shape[1]), np.arange(depth.shape[0]), indexing="xy")
    with np.errstate(invalid="ignore", divide="ignore"):
        xy_var = (np.var(x[mask].astype(dtype)) + np.var(y[mask].astype(dtype))) / dtype(2)
        return dtype(np.sqrt(xy_var / np.var(depth[mask])))


def visualize_normals(depth, acc, scaling=None, dtype=np.float64):
    """-> (rgb, normals, scaling).  The device forms the automatic scaling in float64 and rounds it to float32 once: the float64 result
    here takes that float32 value, so that it is the arbiter of the per-pixel arithmetic."""
    depth = np.asarray(depth, dtype)
    if scaling is None:
        scaling = normals_scaling(depth, dtype)
    scaling = dtype(np.float32(scaling))
    with np.errstate(invalid="ignore", over="ignore"):
        normals = depth_to_normals(scaling * depth, dtype)
        vis = np.isnan(normals).astype(dtype) + np.nan_to_num((normals + dtype(1)) / dtype(2), nan=0.0)
        if acc is not None:
            a = np.asarray(acc, dtype)[:, :, None]
            vis = vis * a + (dtype(1) - a)
    return vis, normals, scaling


def curve(x, name, dtype=np.float64):
    x = np.asarray(x, dtype)
    eps = dtype(EPS)
    with np.errstate(invalid="ignore", divide="ignore"):
        if name == "neg_log":
            return -np.log(x + eps)
        if name == "identity":
            return x
        if name == "reciprocal":
            return dtype(1) / (x + eps)
        if name == "log":
            return np.log(x + eps)
    raise ValueError(name)


def auto_range(depth, acc, ignore_frac, dtype=np.float64):
    """vis.py:75-91 -> (near, far) in dtype: NaN last, equal depths by pixel index; (NaN, NaN) when nothing is kept."""
    d = np.asarray(depth, dtype).reshape(-1)
    a = np.ones_like(d) if acc is None else np.asarray(acc, dtype).reshape(-1)
    a = np.where(np.isnan(d), dtype(0), a)
    order = np.argsort(d, kind="stable")
    ds, cum = d[order], np.cumsum(a[order], dtype=dtype)
    total = cum[-1]
    keep = (cum >= total * dtype(ignore_frac)) & (cum <= total * dtype(1 - ignore_frac))
    if ignore_frac == 0:
        keep[:] = True
    if not keep.any():
        return dtype(np.nan), dtype(np.nan)
    kept = ds[keep]
    return dtype(kept[0] - dtype(EPS)), dtype(kept[-1] + dtype(EPS))


def visualize_depth(depth, acc=None, near=None, far=None, ignore_frac=0, curve_fn="neg_log", modulus=0, dtype=np.float64):
    """-> dict(rgb, value, range=(near, far) before the curve, index: the turbo entry per pixel or None)."""
    depth = np.asarray(depth, dtype)
    a = np.ones_like(depth) if acc is None else np.asarray(acc, dtype)
    a = np.where(np.isnan(depth), dtype(0), a)
    if near is None or far is None:
        n_auto, f_auto = auto_range(depth, acc, ignore_frac, dtype)
    near = n_auto if near is None else dtype(np.float32(near))
    far = f_auto if far is None else dtype(np.float32(far))
    d, n, f = curve(depth, curve_fn, dtype), curve(near, curve_fn, dtype), curve(far, curve_fn, dtype)
    index = None
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if modulus > 0:
            m = dtype(np.float32(modulus))
            value = np.mod(d, m) / m
            colour = sinebow(value, dtype)
        else:
            value = np.nan_to_num(np.clip((d - np.minimum(n, f)) / np.abs(f - n), dtype(0), dtype(1)), nan=0.0)
            index = np.minimum((value * dtype(256)).astype(np.int64), 255)
            colour = turbo_table(dtype)[index]
        rgb = colour * a[:, :, None] + (dtype(1) - a)[:, :, None]
    return dict(rgb=rgb, value=value, range=np.array([near, far], dtype), index=index)


def visualize_suite(depth, acc, dtype=np.float64):
    return {"depth": visualize_depth(depth, acc, dtype=dtype)["rgb"], "depth_mod": visualize_depth(depth, acc, modulus=0.1, dtype=dtype)["rgb"],
            "depth_normals": visualize_normals(depth, acc, dtype=dtype)[0]}
