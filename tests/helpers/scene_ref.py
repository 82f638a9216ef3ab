"""numpy restatement of rnerf_scene_shade (include/rnerf.h) with every float32 operation individually rounded, and the counts of
rnerf_scene_trace taken from the dense march's records.  numpy rounds each float32 array operation once, so writing one operation per
expression gives the kernel's arithmetic; only exp() (float64, one implementation per side) may differ, by at most a float32 ulp of T."""
import numpy as np

F = np.float32


def _axis_coord(s, E):
    """(i0, i1, w) of a face coordinate: u = ((s + 1) 0.5) E - 0.5 clamped to [0, E - 1]."""
    u = (((s + F(1.0)) * F(0.5)) * F(E)) - F(0.5)
    u = np.minimum(np.maximum(u, F(0.0)), F(E - 1)).astype(F)
    f = np.floor(u)
    i0 = f.astype(np.int64)
    i1 = np.minimum(i0 + 1, E - 1)
    return i0, i1, (u - f).astype(F)


def cube_face(d):
    """(face int64 [n] (-1: black: m == 0 or a NaN component), a, b, m float32 [n]) of directions float32 [n, 3]: ties go to x before y
    before z.  cube_lookup also makes a NaN face coordinate black."""
    d = np.asarray(d, F)
    ab = np.abs(d)
    with np.errstate(invalid="ignore"):
        no_nan = ~np.isnan(ab).any(axis=1)                 # no NaN component; an inno_nan one is a direction like any other
        isx = (ab[:, 0] >= ab[:, 1]) & (ab[:, 0] >= ab[:, 2])
        isy = ~isx & (ab[:, 1] >= ab[:, 2])
    axis = np.where(isx, 0, np.where(isy, 1, 2))
    idx = np.arange(d.shape[0])
    m = ab[idx, axis]
    major = d[idx, axis]
    a = d[idx, (axis + 1) % 3]
    b = d[idx, (axis + 2) % 3]
    with np.errstate(invalid="ignore"):
        ok = no_nan & (m > 0)
        face = np.where(ok, 2 * axis + (major < 0), -1)
    return face, a, b, m


def cube_lookup(env, d):
    """env float32 [6, E, E, 3], directions float32 [n, 3] -> rgb float32 [n, 3]."""
    env = np.asarray(env, F)
    E = env.shape[1]
    face, a, b, m = cube_face(d)
    ok = face >= 0
    ms = np.where(ok, m, F(1.0)).astype(F)
    with np.errstate(invalid="ignore"):
        s = (np.where(ok, a, F(0.0)).astype(F) / ms).astype(F)
        t = (np.where(ok, b, F(0.0)).astype(F) / ms).astype(F)
    ok = ok & ~np.isnan(s) & ~np.isnan(t)                  # inf / inf: two inno_nan components have no texel
    s, t = np.where(ok, s, F(0.0)).astype(F), np.where(ok, t, F(0.0)).astype(F)
    u0, u1, wu = _axis_coord(s, E)
    v0, v1, wv = _axis_coord(t, E)
    fc = np.where(ok, face, 0)
    omu, omv = (F(1.0) - wu).astype(F)[:, None], (F(1.0) - wv).astype(F)[:, None]
    wu, wv = wu[:, None], wv[:, None]
    top = (env[fc, v0, u0] * omu) + (env[fc, v0, u1] * wu)
    bot = (env[fc, v1, u0] * omu) + (env[fc, v1, u1] * wu)
    rgb = ((top * omv) + (bot * wv)).astype(F)
    return np.where(ok[:, None], rgb, F(0.0)).astype(F)


def shade(exit_dir, counts, H, W, K, env, step_len, sigma, albedo):
    """-> (rgb float32 [H, W, 3], trans float32 [H, W], mask uint8 [H, W])."""
    d = np.asarray(exit_dir, F).reshape(H * K, W * K, 4)[..., :3]
    c = np.asarray(counts).reshape(2, H * K, W * K)
    e = cube_lookup(env, d.reshape(-1, 3)).reshape(H * K, W * K, 3)
    neg_tau = (-float(sigma)) * float(step_len)
    T = np.exp(neg_tau * c[0].astype(np.float64)).astype(F)
    alb = np.asarray(albedo, np.float64).astype(F)
    colour = ((T[..., None] * e) + ((F(1.0) - T)[..., None] * alb)).astype(F)
    acc = np.zeros((H, W, 3), F)
    acc_t = np.zeros((H, W), F)
    for sy in range(K):
        for sx in range(K):
            acc = (acc + colour[sy::K, sx::K]).astype(F)
            acc_t = (acc_t + T[sy::K, sx::K]).astype(F)
    rcp = F(1.0 / (K * K))
    mask = (c[1].reshape(H, K, W, K) > 0).any(axis=(1, 3))
    return (acc * rcp).astype(F), (acc_t * rcp).astype(F), np.where(mask, 255, 0).astype(np.uint8)


def counts_from_records(path_ior, n_inside, grad_eps):
    """path_ior float32 [N, B, 4] = (n, grad n) -> int32 [2, B]: nodes with n > (float)n_inside, refracting nodes (rnerf_path_summary's
    predicate: the correctly rounded root of (a a + b b) + c c exceeds (float)grad_eps)."""
    ior = np.asarray(path_ior, F)
    with np.errstate(invalid="ignore"):
        inside = (ior[..., 0] > F(n_inside)).sum(axis=0)
        ss = ((ior[..., 1] * ior[..., 1]) + (ior[..., 2] * ior[..., 2])) + (ior[..., 3] * ior[..., 3])
        refr = (np.sqrt(ss.astype(F)) > F(grad_eps)).sum(axis=0)
    return np.stack([inside, refr]).astype(np.int32)
