"""Seeded inputs of the resampler tests (rnerf_resample: resample_depths_kernel<16|4|1> + resample_gather_kernel), shared by
tests/test_resample_cases_host.py and tests/test_gpu_resample_edges.py.  All paths are synthetic: no march, no MLP.

A case is (B, S, P, F, depth family, weight family, u family): B rays, S coarse samples, P path nodes per coarse sample (N = S * P nodes,
one jitter node per group of P as in the models), F fine samples.  build() returns the oracle-shaped arrays [B, N, .], the sample-major
device-shaped ones and the coverage facts that follow from the inputs alone; reference() the oracle's answer (chunked numpy, or the scalar
C reading on the large shapes) and the facts that need it.  Every fact is computed on the CPU from the oracle alone; the tests assert them,
so a case that does not reach its edge fails instead of passing silently.

LDS staging of the depths kernel: need = 4 * S + 2 * F floats per ray; the launcher runs 16 rays per block (need <= 2560, B > 8192),
4 (need <= 10240, B > 1024) or 1 (need <= 40960) and refuses anything larger (csrc/render.hip, rnerf_resample).
"""
from collections import namedtuple

import numpy as np

from oracle import ref_np as R

F32 = np.float32
EPS = float(np.finfo(F32).eps)
NEAR, FAR = 2.0, 6.0

Case = namedtuple("Case", "name B S P F depth weight u seed")

DEPTHS = ("linear", "front", "back", "plateau", "flat")
WEIGHTS = ("rand4", "zero", "zero_from3", "tiny", "overshoot")          # "mixed": ray r takes WEIGHTS[r % 5]
US = ("shared", "stratified", "ties")


def need(c):
    return 4 * c.S + 2 * c.F


def rays_per_block(c):
    """The launcher's choice restated: composite_lanes(B), then the two LDS demotions."""
    rpb = 1 if c.B <= 1024 else (4 if c.B <= 8192 else 16)
    if rpb > 4 and need(c) > 2560:
        rpb = 4
    if rpb > 1 and need(c) > 10240:
        rpb = 1
    return rpb


# ---------------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------------
def _table():
    cs, seed = [], [100]

    def add(group, B, S, P, F, depth, weight, u):
        seed[0] += 1
        cs.append((group, Case("%s-B%d-S%d-P%d-F%d-%s-%s-%s" % (group, B, S, P, F, depth, weight, u), B, S, P, F, depth, weight, u, seed[0])))

    # both sides of each composite_lanes threshold; 1025 = 4 * 256 + 1 and 8193 = 16 * 512 + 1 leave a one-ray tail block
    for B in (1024, 1025, 8192, 8193):
        for u in US:
            add("lanes", B, 12, 5, 40, "linear", "mixed", u)
    add("lanes", 8193, 24, 5, 40, "linear", "overshoot", "stratified")       # every ray's last three inner weights are zero
    # ragged and minimal: one weight (nb = 2) with F = 0, 1, 2; S below every lane count with F no multiple of 4 / 16 / 64; the converse
    for B in (1, 3, 17):
        for F in (0, 1, 2):
            add("ragged", B, 3, 1, F, "linear", "mixed", "shared" if B == 3 else "stratified")
        add("ragged", B, 5, 3, 67, "linear", "mixed", "ties")
        add("ragged", B, 67, 3, 5, "linear", "mixed", "ties")
    # the largest launch of each instantiation: 16 * 2560, 4 * 10240 and 1 * 40960 floats = 163 840 B of dynamic LDS
    add("full_lds", 8193, 15, 1, 1250, "linear", "mixed", "shared")
    add("full_lds", 1025, 10, 1, 5100, "linear", "mixed", "stratified")
    add("full_lds", 2, 3, 1, 20474, "linear", "mixed", "stratified")
    # the launcher's LDS rule: <16> -> <4> (need 2564), <4> -> <1> (10260), and S-heavy (10416): long weight and cdf chains on 64 lanes
    add("demoted", 8193, 16, 1, 1250, "linear", "mixed", "shared")
    add("demoted", 1025, 40, 1, 5050, "linear", "mixed", "stratified")
    add("demoted", 1025, 2600, 1, 8, "linear", "mixed", "ties")
    # the gather: a guess far too high (gallop down), far too low (gallop up), runs of equal node depths, dl == d0
    for B in (300, 1025):
        for P in (5, 1):
            for depth in ("front", "back", "plateau", "flat"):
                add("gather", B, 24, P, 40, depth, "mixed", "ties" if depth in ("plateau", "flat") else "stratified")
    return cs


_TABLE = _table()
CASES = {c.name: c for _, c in _TABLE}
GROUP = {c.name: g for g, c in _TABLE}
REFUSED = Case("refused-S3-F20475", 2, 3, 1, 20475, "linear", "rand4", "shared", 99)          # need = 40962


def names(group=None):
    return [c.name for g, c in _TABLE if group is None or g == group]


def uses_c_reading(c):
    """The dense [B, S - 1, F] mask of the numpy oracle is affordable up to about 1e8 entries; the scalar C reading beyond."""
    return c.B * c.S * c.F > 1e8


def host_names():
    """The cases whose numpy oracle is cheap enough to run twice (numpy and C) in the host test."""
    return [n for n in names() if CASES[n].B * CASES[n].S * CASES[n].F <= 3e7]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle's cdf, with its own lines (ref_np.sorted_piecewise_constant_pdf)
# ---------------------------------------------------------------------------------------------------------------------------------------
def cdf_of(inner):
    """inner weights [B, S - 2] -> (raw float32 running sum before the clamp [B, S - 3], cdf [B, S - 1])."""
    dt = F32
    weight_sum = R._seqsum(inner, axis=-1, keepdims=True)
    padding = np.maximum(dt(0), dt(1e-5) - weight_sum)
    weights = inner + padding / dt(inner.shape[-1])
    weight_sum = weight_sum + padding
    pdf = weights / weight_sum
    raw = np.cumsum(pdf[..., :-1], axis=-1, dtype=F32)
    cdf = np.minimum(dt(1), raw)
    cdf = np.concatenate([np.zeros((inner.shape[0], 1), F32), cdf, np.ones((inner.shape[0], 1), F32)], axis=-1)
    return raw, cdf


# ---------------------------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------------------------
def _depths(c, rng):
    B, N = c.B, c.S * c.P
    k = np.arange(N, dtype=np.float64)[None, :]
    x = k / (N - 1)
    if c.depth in ("linear", "plateau"):
        step = (FAR - NEAR) / N
        z = NEAR + rng.uniform(0, 0.1, (B, 1)) + step * (k + rng.uniform(-0.3, 0.3, (B, N)))
        if c.depth == "plateau":
            q = 3 * step                                              # runs of about three equal node depths
            z = np.round(z / q) * q
    elif c.depth == "front":
        z = NEAR + (4.0 - rng.uniform(0, 0.4, (B, 1))) * x ** 6
    elif c.depth == "back":
        z = FAR - (4.0 - rng.uniform(0, 0.4, (B, 1))) * (1 - x) ** 6
    elif c.depth == "flat":
        z = np.broadcast_to(rng.uniform(NEAR, FAR, (B, 1)), (B, N))
    else:
        raise ValueError(c.depth)
    z = np.ascontiguousarray(z, F32)
    assert (np.diff(z, axis=1) >= 0).all()
    return z


def _weights(c, rng):
    B, S = c.B, c.S
    w = rng.uniform(0, 1, (B, S)).astype(F32) ** 4
    fam = np.arange(B) % len(WEIGHTS) if c.weight == "mixed" else np.full(B, WEIGHTS.index(c.weight))
    w[fam == 1] = 0.0                                                 # the padded-to-uniform branch
    w[fam == 2, 3:] = 0.0                                             # zero-width cdf intervals
    w[fam == 2, :3] = np.maximum(w[fam == 2, :3], F32(1e-4))          # ... whose cdf[1] stays below 1: an interior entry a draw can equal
    w[fam == 3] = 1e-12
    if S >= 6:
        w[fam == 4, S - 4:S - 1] = 0.0                                # last three INNER weights (the inner ones are w[:, 1:S-1]), no padding
    return w, fam


def _stratified(c):
    from samplenerfro_amd import prng
    B, Fn = c.B, c.F
    if Fn == 0:
        return np.zeros((B, 0), F32)
    u = (np.arange(Fn, dtype=F32) * F32(1.0 / Fn))[None] + prng.uniform(prng.PRNGKey(c.seed), (B, Fn), maxval=1.0 / Fn - EPS)
    return np.minimum(u, F32(1 - EPS)).astype(F32)


def _plant_ties(c, u, cdf, rng):
    """Overwrite up to three draws per ray with interior cdf entries of that ray (those the reference's draws can reach: <= 1 - eps), then
    sort along the sample axis.  -> (u, planted): planted = (ray, k) pairs."""
    B, nb = cdf.shape
    if nb < 3 or c.F < 3:
        raise ValueError("planted ties need an interior cdf entry (S >= 4) and F >= 3")
    ks = np.concatenate([np.ones((B, 1), np.int64), rng.integers(1, nb - 1, (B, 2))], axis=1)       # k = 1 and two more in [1, nb - 2]
    fs = np.argsort(rng.random((B, c.F)), axis=1)[:, :3]                                            # three distinct positions per ray
    rows = np.arange(B)[:, None]
    v = cdf[rows, ks]
    ok = v <= F32(1 - EPS)
    u = u.copy()
    u[rows, fs] = np.where(ok, v, u[rows, fs])
    u = np.sort(u, axis=1)
    rr, cc = np.nonzero(ok)
    return u, np.stack([rr, ks[rr, cc]], axis=1)


def count_ties(u, cdf, chunk=512):
    """Per ray: the number of draws f with u[f] == cdf[k] for an interior k (1 <= k <= nb - 2)."""
    B = u.shape[0]
    out = np.zeros(B, np.int64)
    if cdf.shape[1] < 3:
        return out
    for a in range(0, B, chunk):
        out[a:a + chunk] = (u[a:a + chunk, :, None] == cdf[a:a + chunk, None, 1:-1]).any(-1).sum(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# build / reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def build(c):
    """-> dict: z_vals [B,N], pos / dirs [B,N,3], jitter int32 [S], w [B,S], bins [B,S-1], u [B,F], cdf [B,S-1], planted, the device-shaped
    path_pd / path_dr [N,B,4], w_t [S,B], u_dev ([F] shared or [F,B]) and facts."""
    rng = np.random.default_rng(c.seed)
    B, S, P, Fn = c.B, c.S, c.P, c.F
    N = S * P
    z_vals = _depths(c, rng)
    pos = rng.standard_normal((B, N, 3)).astype(F32)
    dirs = R.safe_l2_normalize(rng.standard_normal((B, N, 3)).astype(F32)).astype(F32)
    jitter = (np.arange(0, N, P) + rng.integers(0, P, S)).astype(np.int32)
    w, fam = _weights(c, rng)
    t = z_vals[:, jitter]
    bins = (F32(.5) * (t[:, 1:] + t[:, :-1])).astype(F32)
    raw, cdf = cdf_of(w[:, 1:-1])
    planted = np.zeros((0, 2), np.int64)
    if c.u == "shared":
        u = R.linspace_u(Fn, B)
    elif c.u == "stratified":
        u = _stratified(c)
    elif c.u == "ties":
        u, planted = _plant_ties(c, _stratified(c), cdf, rng)
    else:
        raise ValueError(c.u)
    assert u.dtype == F32 and u.shape == (B, Fn) and (np.diff(u, axis=1) >= 0).all() and (Fn == 0 or (u.min() >= 0 and u.max() <= F32(1 - EPS)))
    over = (raw > 1).any(axis=1) if raw.shape[1] else np.zeros(B, bool)
    facts = {
        "overshoot_rays": int(over.sum()),                            # raw float32 cumsum above 1 before min(1, .)
        "overshoot_family_rays": int((fam == 4).sum()) if S >= 6 else 0,
        "tie_count_per_ray": count_ties(u, cdf) if Fn else np.zeros(B, np.int64),
    }
    if c.depth == "plateau":                                          # runs of >= 2 equal node depths that contain a jitter node
        zj = z_vals[:, jitter]
        lo = np.array([np.searchsorted(z_vals[i], zj[i], "left") for i in range(B)])
        hi = np.array([np.searchsorted(z_vals[i], zj[i], "right") for i in range(B)])
        facts["runs_with_jitter_node"] = int((hi - lo >= 2).sum())
    pd = np.ascontiguousarray(np.concatenate([pos, z_vals[..., None]], -1).transpose(1, 0, 2), F32)
    dr = np.ascontiguousarray(np.concatenate([dirs, np.zeros((B, N, 1), F32)], -1).transpose(1, 0, 2), F32)
    return dict(case=c, z_vals=z_vals, pos=pos, dirs=dirs, jitter=jitter, w=w, bins=bins, u=u, cdf=cdf, planted=planted, facts=facts,
                path_pd=pd, path_dr=dr, w_t=np.ascontiguousarray(w.T), u_dev=np.ascontiguousarray(u[0] if c.u == "shared" else u.T))


def reference_np(d, mask_budget=2e7):
    """oracle.ref_np.sample_pdf, chunked over rays so that the dense mask chunk * (S - 1) * F stays near mask_budget."""
    c = d["case"]
    chunk = max(1, int(mask_budget // max(1, (c.S - 1) * c.F)))
    out = [[], [], [], []]
    for a in range(0, c.B, chunk):
        s = slice(a, a + chunk)
        z, p, dr, _, idx = R.sample_pdf(d["u"][s], d["bins"][s], d["w"][s, 1:-1], d["pos"][s], d["dirs"][s], d["z_vals"][s], d["dirs"][s], d["jitter"])
        for o, x in zip(out, (z, p, dr, idx)):
            o.append(x)
    return tuple(np.concatenate(o, 0) for o in out)


def reference_c(d):
    """The scalar C reading (oracle.c_ref).  Not being able to build or load it is an error, never a skip."""
    from oracle import c_ref as CR
    return CR.sample_pdf(d["u"], d["bins"], d["w"][:, 1:-1], d["pos"], d["dirs"], d["z_vals"], d["jitter"])


def reference(d):
    """-> (z [B,T], pos [B,T,3], dir [B,T,3], idx int32 [B,T]), T = S + F."""
    return reference_c(d) if uses_c_reading(d["case"]) else reference_np(d)


def gather_guess(z_vals, z):
    """resample_gather_kernel's arithmetic first guess of the node count below z, restated in float32 numpy."""
    N = z_vals.shape[1]
    d0, dl = z_vals[:, :1], z_vals[:, -1:]
    inv_step = F32(N - 1) / np.maximum(dl - d0, F32(1e-30))
    gf = (z - d0) * inv_step + F32(1)
    return np.clip(gf, F32(0), F32(N)).astype(np.int64)


def reference_facts(d, z):
    """Facts that need the oracle's merged depths z [B,T]: per ray the number of merged depths equal to two or more node depths, and the
    median distance between the gather's guess and the true searchsorted(z_vals, z, 'left')."""
    zv = d["z_vals"]
    B = zv.shape[0]
    lo = np.stack([np.searchsorted(zv[i], z[i], "left") for i in range(B)])
    hi = np.stack([np.searchsorted(zv[i], z[i], "right") for i in range(B)])
    return {"multi_node_depths_per_ray": (hi - lo >= 2).sum(axis=1),
            "median_guess_error": float(np.median(np.abs(gather_guess(zv, z) - lo)))}


def check_facts(d, z=None):
    """Assert the coverage facts of the case (z: the oracle's merged depths, needed for the plateau / front / back facts)."""
    c, f = d["case"], d["facts"]
    if c.weight == "overshoot" or (c.weight == "mixed" and c.S >= 6 and c.B >= 300):     # a fifth of a mixed batch is of that family
        assert f["overshoot_rays"] >= max(1, int(np.ceil(0.01 * c.B))), "overshoot: %d of %d rays" % (f["overshoot_rays"], c.B)
    if c.u == "ties":
        assert (f["tie_count_per_ray"] >= 1).all(), "planted ties: %d rays without one" % int((f["tie_count_per_ray"] < 1).sum())
    if c.depth == "plateau":
        assert f["runs_with_jitter_node"] >= 1
    if z is not None and c.depth in ("plateau", "front", "back"):
        rf = reference_facts(d, z)
        if c.depth == "plateau":
            assert 2 * int((rf["multi_node_depths_per_ray"] > 0).sum()) >= c.B, "plateau: runs met on %d of %d rays" % (
                int((rf["multi_node_depths_per_ray"] > 0).sum()), c.B)
        else:
            N = c.S * c.P
            assert rf["median_guess_error"] >= N / 8, "%s: median |guess - index| = %g < N / 8 = %g" % (c.depth, rf["median_guess_error"], N / 8)


def device_rows(ref):
    """The oracle's (z, pos, dir, idx) [B,T,.] -> the sample-major records the kernels write: rows_pd [T,B,4], rows_dr [T,B,4], idx [T,B]."""
    z, p, dr, idx = ref
    B, T = z.shape
    pd = np.ascontiguousarray(np.concatenate([p, z[..., None]], -1).transpose(1, 0, 2), F32)
    rd = np.ascontiguousarray(np.concatenate([dr, np.zeros((B, T, 1), F32)], -1).transpose(1, 0, 2), F32)
    return pd, rd, np.ascontiguousarray(idx.T, np.int32)
