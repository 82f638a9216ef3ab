"""numpy restatement of rnerf_path_summary and rnerf_path_plot, written from the definitions in include/rnerf.h.

Records are float32 [N, B, 4]: pd = (x, y, z, dist), dr = (dx, dy, dz, 0), ior = (n, dn/dx, dn/dy, dn/dz).  float32 arithmetic is numpy's
(every operation rounded, sqrt correctly rounded), the optical sum is float64 in ascending node order, pixels are Python integers (so //
is the floor division the header asks for)."""
import math

import numpy as np

F32 = np.float32
BOX, SHADOW, PATH, MARKER = 1, 2, 3, 4
COLOURS = {0: (255, 255, 255), BOX: (255, 0, 0), SHADOW: (139, 206, 151), MARKER: (0, 0, 0)}
LIMIT = float(2 ** 30)


def _sumsq(a, b, c):
    return (a * a + b * b) + c * c


def refracting(ior, grad_eps=1e-3):
    """bool [N, B]: sqrt(sumsq(grad n)) > float32(grad_eps), strict; NaN is not refracting."""
    ior = np.asarray(ior, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(_sumsq(ior[..., 1], ior[..., 2], ior[..., 3])) > F32(grad_eps)


def summary(pd, dr, ior, grad_eps=1e-3):
    """-> (nodes int32 [3, B] = count, first, last; maps float32 [2, B] = bend, optical)."""
    pd, dr, ior = (np.asarray(a, F32) for a in (pd, dr, ior))
    N, B = pd.shape[:2]
    m = refracting(ior, grad_eps)
    count = m.sum(0).astype(np.int32)
    k = np.arange(N)[:, None]
    first = np.where(m, k, N).min(0)
    last = np.where(m, k, -1).max(0)
    first = np.where(count > 0, first, -1).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = dr[N - 1, :, :3] - dr[0, :, :3]
        bend = np.sqrt(_sumsq(d[:, 0], d[:, 1], d[:, 2])).astype(F32)
        opt = np.zeros(B, np.float64)
        for s in range(N - 1):
            e = pd[s, :, :3] - pd[s + 1, :, :3]
            length = np.sqrt(_sumsq(e[:, 0], e[:, 1], e[:, 2])).astype(F32)
            opt = opt + (ior[s, :, 0] - F32(1.0)).astype(np.float64) * length.astype(np.float64)
        optical = opt.astype(F32)
    return np.stack([count, first, last.astype(np.int32)]), np.stack([bend, optical])


def line_pixels(x0, y0, x1, y1):
    """All n + 1 pixels of the segment, n = max(|dx|, |dy|): pixel i = (x0 + (2 i dx + n) // (2 n), y0 + (2 i dy + n) // (2 n))."""
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(x0, y0)]
    return [(x0 + (2 * i * dx + n) // (2 * n), y0 + (2 * i * dy + n) // (2 * n)) for i in range(n + 1)]


def line_pixels_in_panel(x0, y0, x1, y1, size):
    """The pixels of line_pixels that lie in [0, size)^2, visiting only the i whose major coordinate does: at most `size` of them."""
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(x0, y0)] if 0 <= x0 < size and 0 <= y0 < size else []
    c0, dc = (x0, dx) if abs(dx) >= abs(dy) else (y0, dy)
    i0, i1 = (-c0, size - 1 - c0) if dc > 0 else (c0 - (size - 1), c0)
    out = []
    for i in range(max(i0, 0), min(i1, n) + 1):
        x, y = x0 + (2 * i * dx + n) // (2 * n), y0 + (2 * i * dy + n) // (2 * n)
        if 0 <= x < size and 0 <= y < size:
            out.append((x, y))
    return out


def pixel(m, p):
    """(column, row) of the point p under the 2 x 4 matrix m, or None when it cannot be drawn."""
    m = np.asarray(m, np.float64)
    x, y, z = (np.float64(v) for v in p)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((m[0, 0] * x + m[0, 1] * y) + m[0, 2] * z) + m[0, 3]
        v = ((m[1, 0] * x + m[1, 1] * y) + m[1, 2] * z) + m[1, 3]
    if not (abs(u) < LIMIT and abs(v) < LIMIT):          # false for NaN and the infinities
        return None
    return int(math.floor(u)), int(math.floor(v))


def box_edges(box):
    """The 12 edges: edge e runs along axis e // 4 from min to max; bits 0 and 1 of e choose max on the next two axes (cyclically)."""
    lo, hi = np.asarray(box, np.float64)[:3], np.asarray(box, np.float64)[3:]
    out = []
    for e in range(12):
        a = e // 4
        b, c = (a + 1) % 3, (a + 2) % 3
        s, f = lo.copy(), lo.copy()
        f[a] = hi[a]
        s[b] = f[b] = hi[b] if e & 1 else lo[b]
        s[c] = f[c] = hi[c] if e & 2 else lo[c]
        out.append((s, f))
    return out


def plot_keys(pd, ior, rays, panels, size, box=None, floor_z=float("nan"), grad_eps=1e-3):
    """uint32 [P, size, size]: per pixel the largest layer << 28 | id that covers it, 0 where nothing does."""
    pd = np.asarray(pd, F32)
    N, B = pd.shape[:2]
    panels = np.asarray(panels, np.float64)
    keys = np.zeros((panels.shape[0], size, size), np.uint32)
    mark = refracting(ior, grad_eps) if ior is not None else None

    def put(p, x, y, key):
        if 0 <= x < size and 0 <= y < size:
            keys[p, y, x] = max(int(keys[p, y, x]), key)

    def segment(p, a, b, key):
        if a is None or b is None:
            return
        for x, y in line_pixels_in_panel(a[0], a[1], b[0], b[1], size):
            put(p, x, y, key)

    for p, m in enumerate(panels):
        if box is not None:
            for e, (s, f) in enumerate(box_edges(box)):
                segment(p, pixel(m, s), pixel(m, f), BOX << 28 | e)
        for j, ray in enumerate(np.asarray(rays).tolist()):
            if not 0 <= ray < B:
                continue
            for k in range(N):
                a = pd[k, ray, :3]
                qa = pixel(m, a)
                if k + 1 < N:
                    b = pd[k + 1, ray, :3]
                    segment(p, qa, pixel(m, b), PATH << 28 | j)
                    if not math.isnan(floor_z):
                        segment(p, pixel(m, (a[0], a[1], floor_z)), pixel(m, (b[0], b[1], floor_z)), SHADOW << 28 | j)
                if mark is not None and mark[k, ray] and qa is not None:
                    for oy in (-1, 0, 1):
                        for ox in (-1, 0, 1):
                            put(p, qa[0] + ox, qa[1] + oy, MARKER << 28 | j)
    return keys


def plot(pd, ior, rays, ray_rgb, panels, size, box=None, floor_z=float("nan"), grad_eps=1e-3):
    """uint8 [P, size, size, 3]: plot_keys through the colours."""
    keys = plot_keys(pd, ior, rays, panels, size, box, floor_z, grad_eps)
    ray_rgb = np.asarray(ray_rgb, np.uint8).reshape(-1, 3)
    out = np.empty(keys.shape + (3,), np.uint8)
    layer, ident = keys >> 28, keys & 0x0FFFFFFF
    for code, rgb in COLOURS.items():
        out[layer == code] = rgb
    sel = layer == PATH
    out[sel] = ray_rgb[ident[sel]]
    return out
