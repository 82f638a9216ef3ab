"""An independent float64 restatement of visual-hull carving (calib/make_visual_hull.py:107-141) for the tests: a loop over voxel rows
(fixed i, j; the G voxels along z at once) and views, explicit multiplies and adds instead of einsum, np.rint for the rounding.  It shares
no code with samplenerfro_amd/visual_hull.py nor with tests/golden/make_visual_hull_reference.py."""
import numpy as np


def view_matrix(T):
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    out = np.zeros((4, 4))
    for r in range(3):
        for c in range(3):
            out[r, c] = R[c, r]
        out[r, 3] = -(R[0, r] * t[0] + R[1, r] * t[1] + R[2, r] * t[2])
    out[3, 3] = 1.0
    return out


def default_box(transforms):
    """-> (min_point, max_point): the cube of 1.5 x the cameras' largest extent about their mean position."""
    pos = np.stack([np.asarray(T, np.float64)[:3, 3] for T in transforms])
    mid = pos.mean(axis=0)
    side = (pos.max(axis=0) - pos.min(axis=0)).max() * 1.5
    return mid - np.ones(3) * side * 0.5, mid + np.ones(3) * side * 0.5


def projection(cam_mat, T):
    K = np.asarray(cam_mat, np.float64)
    return np.hstack([K, np.zeros((3, 1))]) @ view_matrix(T)


def counts(masks, cam_mat, transforms, G, min_point, max_point):
    """-> int32 [G, G, G], x slowest: the number of views whose mask is set where the voxel centre projects."""
    return counts_pv(masks, [projection(cam_mat, T) for T in transforms], G, min_point, max_point)


def counts_pv(masks, pvs, G, min_point, max_point):
    """counts() from the 3 x 4 projection matrices themselves."""
    masks = [np.asarray(m) for m in masks]
    pvs = [np.asarray(p, np.float64).reshape(3, 4) for p in pvs]
    lin = np.linspace(0, 1, G)
    lo, hi = np.asarray(min_point, np.float64), np.asarray(max_point, np.float64)
    xs, ys, zs = (lin * (hi[a] - lo[a]) + lo[a] for a in range(3))
    out = np.zeros((G, G, G), np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(G):
            for j in range(G):
                for m, p in zip(masks, pvs):
                    H, W = m.shape
                    a = ((p[0, 0] * xs[i] + p[0, 1] * ys[j]) + p[0, 2] * zs) + p[0, 3]
                    b = ((p[1, 0] * xs[i] + p[1, 1] * ys[j]) + p[1, 2] * zs) + p[1, 3]
                    c = ((p[2, 0] * xs[i] + p[2, 1] * ys[j]) + p[2, 2] * zs) + p[2, 3]
                    u = np.minimum(np.maximum(np.rint(a / c), 0), W - 1).astype(np.int64)
                    v = np.minimum(np.maximum(np.rint(b / c), 0), H - 1).astype(np.int64)
                    out[i, j] += m[v, u] > 0
    return out


def grid_values(count, num_views, threshold=0.9):
    """-> float64 [G^3, 1]: 1.33 where count / num_views > threshold, else 1.0 (as 0.33 + 1.0 in float64)."""
    return np.where((np.asarray(count, np.float64) / num_views > threshold).reshape(-1, 1), 0.33 + 1.0, 1.0)
