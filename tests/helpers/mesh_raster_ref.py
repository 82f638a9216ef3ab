"""numpy float64 restatement of rnerf_mesh_depth / rnerf_mask_dilate (include/rnerf.h is the specification), for the tests.

render(): the same projection, edge functions, tie rule, depth interpolation, near / far test and min / lowest-index reduction as the
kernel, every operation an individually rounded float64 one, written as a loop over (groups of) faces, each over the pixels of the 16 x 16 tiles
its bounding box meets.  cast(): an independent brute-force Moeller-Trumbore ray cast in float64 (small inputs only).  dilate() /
bounding_rect(): cv2.dilate with a box and cv2.boundingRect, in numpy.  icosphere(), tetrahedron(): small closed meshes.  The second
half holds the cases the host and the device tests share: cameras, the exact-integer fill-rule cases, the example scene's bars."""
import math
import os

import numpy as np

TILE = 16
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PITCH = 3.0 / 127.0                              # voxel pitch of the example scene's 128^3 grid over [-1.5, 1.5]
EYE4 = np.eye(4, dtype=np.float32)[:3]


def camera(c2w, *, focal=None, cam_mat=None, H=None, W=None, pixel_center=True):
    """-> the keyword arguments of render / cast for the two models of rnerf_generate_rays (Blender with `focal`, OpenCV with `cam_mat`)."""
    pc = 0.5 if pixel_center else 0.0
    if cam_mat is None:
        return dict(c2w=c2w, opencv=0, fx=float(focal), fy=float(focal), cx=W * 0.5, cy=H * 0.5, pc=pc)
    return dict(c2w=c2w, opencv=1, fx=float(cam_mat[0][0]), fy=float(cam_mat[1][1]), cx=float(cam_mat[0][2]), cy=float(cam_mat[1][2]), pc=pc)


def _f32(v):
    return np.float64(np.float32(v))


def project(verts, c2w, opencv, fx, fy, cx, cy):
    """-> X, Y, w (float64 [V]); w = 0 where the vertex cannot be drawn."""
    c = np.asarray(c2w, np.float32)[:3, :4].astype(np.float64)
    R, t = c[:, :3], c[:, 3]
    k = np.empty((3, 3))                                   # cofactors; the inverse is the adjugate over the determinant
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            k[i, j] = R[i1, j1] * R[i2, j2] - R[i1, j2] * R[i2, j1]
    det = (R[0, 0] * k[0, 0] + R[0, 1] * k[0, 1]) + R[0, 2] * k[0, 2]
    Ri = k.T / det
    p = np.asarray(verts, np.float64).reshape(-1, 3)
    d0, d1, d2 = p[:, 0] - t[0], p[:, 1] - t[1], p[:, 2] - t[2]
    xc = (Ri[0, 0] * d0 + Ri[0, 1] * d1) + Ri[0, 2] * d2
    yc = (Ri[1, 0] * d0 + Ri[1, 1] * d1) + Ri[1, 2] * d2
    zc = (Ri[2, 0] * d0 + Ri[2, 1] * d1) + Ri[2, 2] * d2
    sy = sz = 1.0 if opencv else -1.0
    depth = sz * zc
    with np.errstate(all="ignore"):
        X = (xc * _f32(fx)) / depth + _f32(cx)
        Y = ((sy * yc) * _f32(fy)) / depth + _f32(cy)
        w = 1.0 / depth
        ok = (depth > 0.0) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(w) & (w > 0.0)
    return X, Y, np.where(ok, w, 0.0)


def _edge(P, Q, sgn):
    """Per face: (px, py, dx, dy, s, tie) of the edge P -> Q; P, Q: (X [F], Y [F])."""
    dxo, dyo = (Q[0] - P[0]) * sgn, (Q[1] - P[1]) * sgn
    swap = (Q[0] < P[0]) | ((Q[0] == P[0]) & (Q[1] < P[1]))
    px, py = np.where(swap, Q[0], P[0]), np.where(swap, Q[1], P[1])
    qx, qy = np.where(swap, P[0], Q[0]), np.where(swap, P[1], Q[1])
    return px, py, qx - px, qy - py, np.where(swap, -sgn, sgn), (dyo > 0.0) | ((dyo == 0.0) & (dxo < 0.0))


def _first(lo, pc, n):
    return np.minimum(np.maximum(np.ceil(lo - pc) - 1.0, 0.0), float(n)).astype(np.int64)


def _last(hi, pc, n):
    return np.minimum(np.maximum(np.floor(hi - pc) + 1.0, -1.0), float(n - 1)).astype(np.int64)


def render(verts, faces, H, W, *, c2w, opencv, fx, fy, cx, cy, pc=0.5, znear=0.1, zfar=100.0, depth64=False):
    """-> depth float32 [H, W] (0 = nothing; depth64: before that rounding), tri int32 [H, W] (-1 = nothing), hits int32 [H, W], skipped (int)."""
    X, Y, w = project(verts, c2w, opencv, fx, fy, cx, cy)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    pc = _f32(pc)
    best = np.full((H, W), np.inf)
    tri = np.full((H, W), -1, np.int32)
    hits = np.zeros((H, W), np.int32)
    if len(f) == 0:
        return np.zeros((H, W), np.float32), tri, hits, 0
    A, B, C = [(X[f[:, k]], Y[f[:, k]]) for k in range(3)]
    wA, wB, wC = w[f[:, 0]], w[f[:, 1]], w[f[:, 2]]
    bad = (wA == 0.0) | (wB == 0.0) | (wC == 0.0)
    with np.errstate(all="ignore"):
        area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
        sgn = np.where(area > 0.0, 1.0, -1.0)
        E = [_edge(A, B, sgn), _edge(B, C, sgn), _edge(C, A, sgn)]
        xs, ys = np.stack([A[0], B[0], C[0]]), np.stack([A[1], B[1], C[1]])
        xs, ys = np.where(bad, 0.0, xs), np.where(bad, 0.0, ys)
        c0, c1 = _first(xs.min(0), pc, W), _last(xs.max(0), pc, W)
        r0, r1 = _first(ys.min(0), pc, H), _last(ys.max(0), pc, H)
    draw = ~bad & (c0 <= c1) & (r0 <= r1) & ((area > 0.0) | (area < 0.0))
    c0, r0 = (c0 // TILE) * TILE, (r0 // TILE) * TILE                          # the pixels of the tiles the box meets
    c1, r1 = np.minimum((c1 // TILE) * TILE + TILE - 1, W - 1), np.minimum((r1 // TILE) * TILE + TILE - 1, H - 1)
    # faces whose tile ranges have one shape are evaluated together, a few million (face, pixel) pairs at a time
    idx = np.nonzero(draw)[0]
    shape_key = (r1[idx] - r0[idx] + 1) * (W + TILE) + (c1[idx] - c0[idx] + 1)
    hit_pix, hit_d, hit_f = [], [], []
    for key in np.unique(shape_key):
        group = idx[shape_key == key]
        nh, nw = int(key // (W + TILE)), int(key % (W + TILE))
        step = max(1, (1 << 21) // (nh * nw))
        for g0 in range(0, len(group), step):
            i = group[g0:g0 + step]
            col = c0[i][:, None, None] + np.arange(nw)[None, None, :]
            row = r0[i][:, None, None] + np.arange(nh)[None, :, None]
            x, y = col.astype(np.float64) + pc, row.astype(np.float64) + pc
            e = []
            inside = np.ones((len(i), nh, nw), bool)
            for px, py, dx, dy, s, tie in E:
                k = lambda a: a[i][:, None, None]
                v = (k(dx) * (y - k(py)) - k(dy) * (x - k(px))) * k(s)
                inside &= (v > 0.0) | ((v == 0.0) & k(tie))
                e.append(v)
            eab, ebc, eca = e
            esum = (eab + ebc) + eca
            with np.errstate(all="ignore"):
                d = esum / ((ebc * wA[i][:, None, None] + eca * wB[i][:, None, None]) + eab * wC[i][:, None, None])
            m = inside & (esum > 0.0) & (znear < d) & (d < zfar)
            fi, ri, ci = np.nonzero(m)
            hit_pix.append((row[fi, ri, 0] * W + col[fi, 0, ci]).astype(np.int64)); hit_d.append(d[fi, ri, ci]); hit_f.append(i[fi])
    skipped = int(bad.sum())
    if hit_pix:
        pix, dd, ff = np.concatenate(hit_pix), np.concatenate(hit_d), np.concatenate(hit_f)
        hits = np.bincount(pix, minlength=H * W).astype(np.int32).reshape(H, W)
        order = np.lexsort((ff, dd, pix))                                     # per pixel: the smallest depth, then the lowest face index
        first = order[np.concatenate([[True], pix[order][1:] != pix[order][:-1]])] if len(order) else order
        best.reshape(-1)[pix[first]] = dd[first]
        tri.reshape(-1)[pix[first]] = ff[first].astype(np.int32)
    depth = np.where(hits > 0, best, 0.0)
    return depth if depth64 else depth.astype(np.float32), tri, hits, skipped


def rays(H, W, *, c2w, opencv, fx, fy, cx, cy, pc=0.5):
    """The rays of rnerf_generate_rays in float64, not normalised: the camera-space direction has view-axis component 1, so the ray
    parameter IS the distance along the view axis.  -> origin [3], directions [H, W, 3]."""
    c = np.asarray(c2w, np.float32)[:3, :4].astype(np.float64)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    fx, fy, cx, cy, pc = (_f32(v) for v in (fx, fy, cx, cy, pc))
    if opencv:
        cam = np.stack([(col - cx + pc) / fx, (row - cy + pc) / fy, np.ones_like(col)], -1)
    else:
        cam = np.stack([(col + pc - cx) / fx, -(row + pc - cy) / fy, -np.ones_like(col)], -1)
    return c[:, 3], cam @ c[:, :3].T


def cast(verts, faces, H, W, *, znear=0.1, zfar=100.0, **cam):
    """Brute force: every ray against every face (Moeller-Trumbore, float64, no tie rule).  -> depth float64 [H, W] (0 = nothing), hits."""
    o, d = rays(H, W, **cam)
    d = d.reshape(-1, 3)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    best = np.full(len(d), np.inf)
    hits = np.zeros(len(d), np.int32)
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3):
        e1, e2 = v[b] - v[a], v[c] - v[a]
        p = np.cross(d, e2)
        det = p @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            s = o - v[a]
            u = (p @ s) * inv
            q = np.cross(s, e1)
            vv = (d @ q) * inv
            t = (q @ e2) * inv
        m = (det != 0.0) & (u >= 0.0) & (vv >= 0.0) & (u + vv <= 1.0) & (znear < t) & (t < zfar)
        hits += m
        best = np.where(m & (t < best), t, best)
    return np.where(hits > 0, best, 0.0).reshape(H, W), hits.reshape(H, W)


def edge_distance(verts, faces, rows, cols, *, c2w, opencv, fx, fy, cx, cy, pc=0.5):
    """Smallest distance, in pixels, from the sample points of pixels (rows[i], cols[i]) to any projected edge of the mesh."""
    X, Y, _ = project(verts, c2w, opencv, fx, fy, cx, cy)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]); b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    P, Q = np.stack([X[a], Y[a]], -1), np.stack([X[b], Y[b]], -1)
    out = []
    for r, c in zip(rows, cols):
        s = np.array([c + pc, r + pc])
        u = np.clip(((s - P) * (Q - P)).sum(-1) / np.maximum(((Q - P) ** 2).sum(-1), 1e-300), 0.0, 1.0)
        out.append(np.sqrt(((P + u[:, None] * (Q - P) - s) ** 2).sum(-1)).min())
    return np.array(out)


def dilate(mask, ky, kx):
    """cv2.dilate(mask, np.ones((ky, kx)), iterations=1) with cv2's defaults: anchor at the centre, nothing outside the image. -> 0 / 255."""
    m = np.asarray(mask) > 0
    H, W = m.shape
    rows = np.zeros_like(m)
    for k in range(-(kx // 2), kx // 2 + 1):
        lo, hi = max(0, -k), min(W, W - k)
        if lo < hi:
            rows[:, lo:hi] |= m[:, lo + k:hi + k]
    out = np.zeros_like(m)
    for k in range(-(ky // 2), ky // 2 + 1):
        lo, hi = max(0, -k), min(H, H - k)
        if lo < hi:
            out[lo:hi] |= rows[lo + k:hi + k]
    return out.astype(np.uint8) * 255


def bounding_rect(mask):
    """cv2.boundingRect of mask > 0: (x, y, w, h); (0, 0, 0, 0) when nothing is set."""
    r, c = np.nonzero(np.asarray(mask) > 0)
    if len(r) == 0:
        return (0, 0, 0, 0)
    return (int(c.min()), int(r.min()), int(c.max() - c.min() + 1), int(r.max() - r.min() + 1))


def tetrahedron():
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def icosphere(subdivisions=1):
    """A unit icosahedron, each face split in four `subdivisions` times (80 faces at 1): closed and consistently oriented."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v), np.array(f, np.int32)


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), opencv=False):
    """camera-to-world [3, 4] float32 of a camera at `eye` looking at `target` (Blender: looks along -z, y up; OpenCV: along +z, y down)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye; fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    R = np.stack([right, -upv, fwd], 1) if opencv else np.stack([right, upv, -fwd], 1)
    return np.concatenate([R, eye[:, None]], 1).astype(np.float32)


def sphere_cameras(H, W):
    """Both camera models on the unit icosphere, off-centre principal point and fx != fy for the OpenCV one."""
    blender = camera(look_at((2.2, -1.7, 1.1)), focal=0.9 * W, H=H, W=W)
    opencv = camera(look_at((2.2, -1.7, 1.1), opencv=True), cam_mat=[[0.9 * W, 0, 0.46 * W], [0, 1.1 * W, 0.55 * H], [0, 0, 1]])
    return {"blender": blender, "opencv": opencv}


# ---- fill-rule cases: an OpenCV camera at the identity pose and a mesh in the plane z = fx = fy, so vertex (x, y, z) projects to exactly
# (x + cx, y + cy) and every edge function is an exact integer (or half-integer) computation
FOCAL = 32.0


def convex_masks(poly, H, W):
    """(strictly inside, strictly outside) [H, W] of the samples (c + 0.5, r + 0.5) for a convex polygon; exact (small half-integers)."""
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    cr = np.stack([(q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0]) for p, q in zip(poly, np.roll(poly, -1, 0))])
    if cr.sum() < 0:
        cr = -cr
    return (cr > 0).all(0), (cr < 0).any(0)


def planar_cases():
    """name -> (verts [V, 2] in PIXEL coordinates (X, Y), faces, outline) at H x W = 24 x 40, pixel_center on: pixel (r, c) samples
    (c + 0.5, r + 0.5)."""
    H, W = 24, 40
    out = {}
    # a quad with integer corners (no sample on its border), split along the diagonal x - y = 1, which runs through 16 samples
    quad_v = np.array([[4.0, 3.0], [20.0, 3.0], [20.0, 19.0], [4.0, 19.0]])
    out["quad"] = (quad_v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), quad_v)
    # a six-triangle fan around a vertex on the sample of pixel (12, 20); the spokes along y = 12.5 run through samples too
    cx, cy = 20.5, 12.5
    ring = np.array([[cx + 9, cy], [cx + 4, cy + 8], [cx - 5, cy + 8], [cx - 9, cy], [cx - 4, cy - 8], [cx + 5, cy - 8]])
    fan_v = np.concatenate([[[cx, cy]], ring])
    out["fan"] = (fan_v, np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32), ring)
    return H, W, out


def planar_run(render, name, reverse, blender):
    """Run one planar case through `render(verts3, faces, H, W, cam)`; -> (its result, samples strictly inside, strictly outside)."""
    H, W, cases_ = planar_cases()
    v2, f, outline = cases_[name]
    f = f[:, ::-1].copy() if reverse else f
    cxp, cyp = 0.0, 0.0                                   # principal point at the image origin: X = x, Y = y
    if blender:                                            # Blender: cx = W / 2, cy = H / 2, y up, looks along -z
        v3 = np.stack([v2[:, 0] - W * 0.5, -(v2[:, 1] - H * 0.5), np.full(len(v2), -FOCAL)], 1)
        cam = camera(EYE4, focal=FOCAL, H=H, W=W)
    else:
        v3 = np.stack([v2[:, 0] - cxp, v2[:, 1] - cyp, np.full(len(v2), FOCAL)], 1)
        cam = camera(EYE4, cam_mat=[[FOCAL, 0, cxp], [0, FOCAL, cyp], [0, 0, 1]])
    return (render(v3, f, H, W, cam),) + convex_masks(outline, H, W)


def check_planar(run):
    """run(name) -> ((depth, tri, hits, skipped), inside, outside) for the cases "quad" and "fan"."""
    (depth, tri, hits, skipped), inside, outside = run("quad")
    assert skipped == 0 and inside.sum() == 256 and np.all(inside | outside)  # no sample on the quad's border
    assert np.array_equal(hits, inside.astype(np.int32))                      # once on the diagonal, once elsewhere inside, never outside
    assert np.all(depth[inside] == np.float32(FOCAL)) and np.all(depth[outside] == 0)
    assert set(np.unique(tri[inside])) == {0, 1} and np.all(tri[outside] == -1)
    (depth, tri, hits, skipped), inside, outside = run("fan")
    assert skipped == 0 and inside[12, 20] and hits[12, 20] == 1              # the fan's centre vertex sits on the sample of pixel (12, 20)
    assert np.all(hits[inside] == 1) and np.all(hits[outside] == 0) and hits.max() == 1
    assert len(np.unique(tri[inside])) == 6 and np.all(depth[hits == 1] == np.float32(FOCAL))


def example_camera():
    import cases
    H = W = 800
    focal = 0.5 * W / math.tan(0.5 * cases.EXAMPLE_CAMERA_ANGLE_X)
    return H, W, focal, camera(cases.EXAMPLE_C2W, focal=focal, H=H, W=W)


def check_example(depth, hits):
    """depth float32 [800, 800], hits int32 [800, 800] of the example OBJ from the example camera, against Blender's depth pass."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_depth.npz"))
    zz, rows, cols = z["z"].astype(np.float64), z["rows"], z["cols"]
    d = depth[rows][:, cols].astype(np.float64)
    h = hits[rows][:, cols]
    blender_hit, hit = zz < 1e9, d > 0
    agree = float((blender_hit == hit).mean())
    both = blender_hit & hit
    err = (d[both] - zz[both]) / PITCH
    odd_fixture, odd_frame = int((h % 2 == 1).sum()), int((hits % 2 == 1).sum())
    print(f"example OBJ vs Blender's depth pass: silhouette agreement {agree:.4f}, depth error median {np.median(err):+.3f}, "
          f"p95 |e| {np.percentile(np.abs(err), 95):.3f}, max |e| {np.abs(err).max():.3f} pitches on {int(both.sum())} pixels; "
          f"odd hit counts: {odd_fixture} of {h.size} fixture pixels, {odd_frame} of the whole frame")
    assert h.size == 10000
    assert agree > 0.99
    assert abs(np.median(err)) < 0.3 and np.percentile(np.abs(err), 95) < 0.5 and np.abs(err).max() < 2.0
    assert odd_fixture == 0
