"""BASELINE.json's full sizes (4096 rays x 128 samples, N = 1536 eikonal steps, 512^3 grid) through size-independent
properties: the oracle would take minutes here, so each test checks something the domain guarantees at any size."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from samplenerfro_amd import synthetic as syn

pytestmark = pytest.mark.gpu
B, S, P, G = 4096, 128, 12, 512
N = S * P


@pytest.fixture(scope="module")
def world():
    from samplenerfro_amd import models
    from samplenerfro_amd.utils import Rays
    dev = torch.device("cuda:0")
    out = {}
    for name, radius in (("vacuum", 0.0), ("sphere", 0.6)):
        if radius > 0:
            a = torch.linspace(-1.5, 1.5, G, dtype=torch.float64, device=dev)
            r = torch.sqrt(a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2)
            grid = (1.0 + 0.5 * torch.clamp((radius - r) / (3.0 / (G - 1)) + 0.5, 0.0, 1.0)).float()
            del r
        else:
            grid = torch.ones((G, G, G), device=dev)
        out[name] = models.NerfModel(ndim=[G] * 3, nmin=[-1.5] * 3, nmax=[1.5] * 3, grid=grid, num_coarse_samples=S, num_fine_samples=256,
                                     num_path_samples=P, device=dev)
        del grid
    pf = syn.init_params_flat(0, fine=True, bias_scale=0.05)
    out["variables"] = models.make_variables({k: torch.from_numpy(v).to(dev) for k, v in pf.items()})
    o, d = syn.sphere_rays(B)
    out["rays"] = Rays(torch.from_numpy(o).to(dev), None, torch.from_numpy(d).to(dev), None)
    return out


def test_vacuum_march_is_repeated_addition(world):
    """KAT 1: n = 1, grad n = 0  =>  rp_k by k repeated fp32 additions of fl(step * d), dir constant, dist by repeated
    addition of the step length — bit-exact at 4096 x 1536."""
    from samplenerfro_amd import ops
    m, rays = world["vacuum"], world["rays"]
    pd, dr, _, _ = ops.march(m.table, m.spec, rays.origins, rays.viewdirs, m.near, m.far, N)
    step = torch.tensor(np.float32((m.far - m.near) / (N - 1)), device=pd.device)
    d = rays.viewdirs
    p = rays.origins + torch.tensor(np.float32(m.near), device=pd.device) * d
    inc = (step / torch.ones_like(d[:, :1])) * d                         # (step / n) * rd with n == 1
    t = torch.full((B,), np.float32(m.near), device=pd.device)
    nrm = torch.sqrt(torch.clamp((d * d)[:, 0] + (d * d)[:, 1] + (d * d)[:, 2], min=1e-6))
    dn = d / nrm[:, None]
    for k in range(N):
        if k in (0, 1, 2, 7, 100, 777, N - 1):
            assert torch.equal(pd[k, :, :3], p) and torch.equal(pd[k, :, 3], t) and torch.equal(dr[k, :, :3], dn)
        q = p + inc
        dl = p - q
        t = t + torch.sqrt((dl * dl)[:, 0] + (dl * dl)[:, 1] + (dl * dl)[:, 2])
        p = q


def test_rays_are_independent(world):
    """Permuting the rays of a batch permutes the outputs bit-exactly (march, MLP tiles, compositing, resampling: no cross-ray term)."""
    m, v, rays = world["sphere"], world["variables"], world["rays"]
    key = np.array([0, 42], np.uint32)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(rays.origins.device)
    ret_a, _ = m.apply(v, key, key, rays, False)
    ret_b, _ = m.apply(v, key, key, type(rays)(rays.origins[perm].contiguous(), None, rays.viewdirs[perm].contiguous(), None), False)
    for la, lb in zip(ret_a, ret_b):
        for a, b in zip(la, lb):
            assert torch.equal(a[perm], b)


def test_compositing_invariants_and_sorted_resampling(world):
    m, v, rays = world["sphere"], world["variables"], world["rays"]
    key = np.array([0, 7], np.uint32)
    taps = {}
    ret, _ = m.apply(v, key, key, rays, True, taps=taps)
    for lvl, wname in ((0, "weights_c"), (1, "weights_f")):
        rgb, dist, acc, trans, tb = ret[lvl]
        w = taps[wname]
        assert torch.isfinite(rgb).all() and torch.isfinite(dist).all()
        assert float((w.sum(0) + trans.reshape(-1) - 1).abs().max()) < 2e-5          # partition of unity: sum w + T_last = 1
        assert float((acc - w.sum(0)).abs().max()) < 1e-5
        assert float(rgb.min()) >= -0.001 - 1e-5 and float(rgb.max()) <= 1.001 + 1e-5  # convex combination of padded sigmoids / bkgd
        assert bool((w >= 0).all())
    z = taps["rows_pd"][..., 3]                                                        # merged coarse + fine depths, [S+F, B]
    assert bool((z[1:] >= z[:-1]).all())
    idx = taps["idx_f"].long()
    assert int(idx.min()) >= 0 and int(idx.max()) <= N - 1
    zn = taps["path_pd"][..., 3]                                                       # node depths [N, B]
    cols = torch.arange(B, device=z.device)[None, :]
    lo = zn[idx, cols]
    hi = zn[torch.clamp(idx + 1, max=N - 1), cols]
    assert bool((z >= lo).all())                                                       # idx = max(searchsorted_left - 1, 0)
    inner = (idx + 1 <= N - 1) & (z > zn[0][None, :])
    assert bool((z[inner] <= hi[inner]).all())
    assert bool(((z > lo) | (idx == 0))[z > zn[0][None, :]].all())                     # 'left': z equal to a node depth maps to the node before


def test_gradient_is_the_mean_of_the_half_batch_gradients():
    """mse terms are means over rays: grad(batch) = (grad(first half) + grad(second half)) / 2 — a checksum of the whole
    backward path (different tile / workgroup decompositions) at the full 4096 x 128 size."""
    from samplenerfro_amd import models, utils as U
    from samplenerfro_amd.train import TrainState, train_step
    from samplenerfro_amd.utils import Rays
    dev = torch.device("cuda:0")
    Gs = 64
    flags = U.default_flags(num_coarse_samples=S, num_fine_samples=0, num_path_samples=P, white_bkgd=False, bg_weight=0.0, bg_smooth_weight=0.0,
                            use_online_sparsity=False, randomized=False)
    model, variables = models.construct_nerf(np.array([0, 3], np.uint32), None, flags, [Gs] * 3, [-1.5] * 3, [1.5] * 3,
                                             torch.ones((Gs, Gs, Gs), device=dev))
    pf = syn.init_params_flat(3, fine=False, bias_scale=0.05)
    for k in ("coarse_mlp", "bkgd_mlp"):
        variables["flat"][k].copy_(torch.from_numpy(pf[k]).to(dev))
    o, d = syn.sphere_rays(B, seed=11)
    pix = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (B, 3)).astype(np.float32)).to(dev)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    jitter = np.arange(0, N, P) + 5
    grads = []
    for lo, hi in ((0, B), (0, B // 2), (B // 2, B)):
        state = TrainState.create(model, variables, flags)
        taps = {}
        train_step(model, np.array([1, 1], np.uint32), state, {"rays": Rays(o[lo:hi].contiguous(), None, d[lo:hi].contiguous(), None),
                                                               "pixels": pix[lo:hi].contiguous(), "annealed_alpha": 0.0}, jitter=jitter, taps=taps)
        grads.append(taps["grads"].double())
    full, halves = grads[0], 0.5 * (grads[1] + grads[2])
    cos = float((full * halves).sum() / (full.norm() * halves.norm()))
    err = float((full - halves).abs().max() / full.abs().max())
    print(f"full vs mean-of-halves gradient: cosine {cos:.7f}, max err / max |g| {err:.2e}")
    assert cos > 0.99999 and err < 2e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# BASELINE configs 4 (dolphin) and 5 (glass) at their full sizes.  The oracle cannot march 8192 x 6144 nodes in test time, but rays are
# independent (test_rays_are_independent): a SAMPLE of the rays of the full-size batch is marched / rendered by the oracle on the very
# table the device built (384^3 / 256^3), and the full batch must reproduce those rays bit for bit (path) / within 1e-4 (RGB, depth).
# ---------------------------------------------------------------------------------------------------------------------------------
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def _ball_grid_dev(G, nmin, nmax, radius, ri, ksize, ksigma, dev):
    from samplenerfro_amd import ops
    ax = [torch.linspace(nmin[i], nmax[i], G, dtype=torch.float64, device=dev) for i in range(3)]
    c = [0.5 * (nmin[i] + nmax[i]) for i in range(3)]
    r = torch.sqrt((ax[0][:, None, None] - c[0]) ** 2 + (ax[1][None, :, None] - c[1]) ** 2 + (ax[2][None, None, :] - c[2]) ** 2)
    h = (nmax[0] - nmin[0]) / (G - 1)
    raw = 1.0 + 0.33 * torch.clamp((radius - r) / h + 0.5, 0.0, 1.0)
    del r
    return ops.grid_prefilter(((raw - 1.0) * ri / 0.33 + 1.0).float(), ksize, ksigma), c


def _opencv_frame(c2w, H, W, cam, dev):
    from samplenerfro_amd import ops
    o, _, v = ops.generate_rays(c2w, H, W, dev, cam_mat=cam)
    return o.reshape(-1, 3), v.reshape(-1, 3)


def _oracle_sample(model, pf, o, v, jitter, sel, cfg_kw, u=None):
    """The oracle on rays `sel` of the batch, with the device-built table as its grid input."""
    from oracle import ref_np as R
    table = model.table.cpu().numpy().reshape(-1, 4)
    mc = R.ModelConfig(model.ndim, model.nmin, model.nmax, near=model.near, far=model.far, num_coarse_samples=model.num_coarse_samples,
                       num_fine_samples=model.num_fine_samples, num_path_samples=model.num_path_samples)
    for k, val in cfg_kw.items():
        setattr(mc, k, val)
    taps = {}
    ret, _ = R.nerf_forward(mc, syn.params_tree(pf), table, o[sel].cpu().numpy(), v[sel].cpu().numpy(), jitter, u_fine=u, taps=taps)
    return ret, taps


def test_stage_all_march_full_size(world):
    """E1/E2 with stage "all*" at 4096 rays x 1536 nodes on the 512^3 sphere: so3_mlp is evaluated by four waves per 32-ray block that
    exchange activations through LDS (one barrier per exchange) — a missed barrier would show up as run-to-run differences, so two
    runs must agree bit for bit, in the given ray order and in the shell-coherent order (rays are independent: the order changes no
    value); 8 rays against the oracle's stage-all path_sampler on the device-built table."""
    from oracle import ref_np as R
    from samplenerfro_amd import ops
    shapes = [(60, 128), (128, 128), (128, 128), (188, 128), (128, 3)]
    m, rays = world["sphere"], world["rays"]
    rng = np.random.default_rng(21)
    flat = syn.init_mlp_flat(rng, shapes, 0.05)
    flat[-(128 * 3 + 3):-3] = (0.05 * rng.standard_normal(128 * 3)).astype(np.float32)      # a visible rotation (init is N(0, 1e-5))
    so3 = torch.from_numpy(flat).to(rays.origins.device)
    alpha = 0.8
    runs = [ops.march_all(m.table, m.spec, so3, rays.origins, rays.viewdirs, m.near, m.far, N, alpha, False, coherent) for coherent in (False, False, True)]
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])
    pd, dr, _ = runs[0]
    pd0, _, _, _ = ops.march(m.table, m.spec, rays.origins, rays.viewdirs, m.near, m.far, N)
    moved = (pd[-1, :, :3] - pd0[-1, :, :3]).abs().amax(-1)
    assert int((moved > 1e-3).sum()) > 500                               # so3_mlp really bends the rays that cross the sphere
    idx_b = torch.nonzero(moved > 1e-3).reshape(-1)
    idx_m = torch.nonzero(moved == 0).reshape(-1)
    sel = torch.cat([idx_b[:: max(len(idx_b) // 6, 1)][:6], idx_m[:2]]).cpu().numpy()
    table = m.table.cpu().numpy().reshape(-1, 4)
    o, d = rays.origins.cpu().numpy()[sel], rays.viewdirs.cpu().numpy()[sel]
    rp, rd, rt, _, _ = R.path_sampler(o, d, table, m.ndim, m.nmin, m.nmax, m.near, m.far, N, so3_params=syn.flat_to_np_tree(flat, shapes), annealed_alpha=alpha)
    got_p = pd[:, sel, :3].cpu().numpy().transpose(1, 0, 2); got_t = pd[:, sel, 3].cpu().numpy().T; got_d = dr[:, sel, :3].cpu().numpy().transpose(1, 0, 2)
    ep, et, ed = np.abs(got_p - rp).max(), np.abs(got_t - rt).max(), np.abs(got_d - rd).max()
    print(f"stage-all march 4096 x 1536 vs the oracle on 8 rays: position {ep:.2e}, depth {et:.2e}, direction {ed:.2e}")
    assert ep < 1e-4 and et < 1e-4 and ed < 1e-4
    assert np.array_equal(got_p[6:], rp[6:])                             # rays outside the shell never see the MLP: bit-exact


def test_config5_glass_full_size_chunk():
    """One render_image chunk of config 5: 8192 OpenCV rays, flat S = 256, P = 24 (N = 6144 eikonal steps), G = 384 anisotropic glass bbox,
    prefilter (5, 3.0).  24 rays of the chunk against the oracle (bit-exact path and voxel walk, RGB / depth 1e-4), the chunk's invariants."""
    import cases as CS
    from samplenerfro_amd import models
    from samplenerfro_amd.utils import Rays
    dev = torch.device("cuda:0")
    G, Sg, Pg, Bg = 384, 256, 24, 8192
    nmin, nmax = CS.GLASS_BBOX
    grid, c = _ball_grid_dev(G, nmin, nmax, 0.8, 0.33, 5, 3.0, dev)
    model = models.NerfModel(ndim=[G] * 3, nmin=nmin, nmax=nmax, grid=grid, near=0.2, far=14.0, num_coarse_samples=Sg, num_fine_samples=0,
                             num_path_samples=Pg, device=dev)
    del grid
    pf = syn.init_params_flat(52, fine=False, bias_scale=0.05)
    variables = models.make_variables({k: torch.from_numpy(val).to(dev) for k, val in pf.items()})
    o, v = _opencv_frame(CS._look_at([c[0] + 3.2, c[1] - 3.4, c[2] + 1.4], c), 800, 800, [[875.0, 0.0, 399.6], [0.0, 880.0, 400.2], [0.0, 0.0, 1.0]], dev)
    lo = 400 * 800 - Bg // 2                                             # a chunk around the image centre: its rays cross the object
    o, v = o[lo:lo + Bg].contiguous(), v[lo:lo + Bg].contiguous()
    key = np.array([0, 5], np.uint32)
    taps = {}
    ret, _ = model.apply(variables, key, key, Rays(o, None, v, None), False, taps=taps)
    rgb, dist, acc, trans, tb = ret[0]
    w = taps["weights_c"]
    assert torch.isfinite(rgb).all() and torch.isfinite(dist).all()
    assert float((w.sum(0) + trans.reshape(-1) - 1).abs().max()) < 5e-5
    zn = taps["path_pd"][..., 3]
    assert zn.shape == (Sg * Pg, Bg) and bool((zn[1:] > zn[:-1]).all())                       # arc length strictly increases
    assert float(taps["path_ior"][..., 0].max()) > 1.3                                         # the chunk really crosses the glass ball
    sel = torch.arange(0, Bg, Bg // 24, device=dev)[:24]
    oret, otaps = _oracle_sample(model, pf, o, v, taps["jitter"], sel, {})
    sel_c = sel.cpu().numpy()
    pd = taps["path_pd"][:, sel].cpu().numpy()
    assert np.array_equal(pd[..., :3].transpose(1, 0, 2), otaps["ray_pos"]) and np.array_equal(pd[..., 3].T, otaps["ray_dist"])
    assert np.array_equal(taps["path_dr"][:, sel].cpu().numpy()[..., :3].transpose(1, 0, 2), otaps["ray_dir"])
    for got, want in zip((rgb, dist, acc), oret[0][:3]):
        assert float(np.abs(got[sel].cpu().numpy() - want).max()) < 1e-4
    # the same 24 rays rendered alone: bit-identical to their values inside the 8192-ray chunk
    ret_s, _ = model.apply(variables, key, key, Rays(o[sel].contiguous(), None, v[sel].contiguous(), None), False)
    for a, b in zip(ret_s[0], ret[0]):
        assert torch.equal(a, b[sel])
    assert sel_c.size == 24


def _dolphin_world(B, dev):
    import cases as CS
    from samplenerfro_amd import models, utils as U
    from samplenerfro_amd.train import TrainState
    from samplenerfro_amd.utils import Rays
    G = 256
    nmin, nmax = CS.DOLPHIN_BBOX
    grid, c = _ball_grid_dev(G, nmin, nmax, 0.1, 0.33, 5, 1.0, dev)
    flags = U.default_flags(num_coarse_samples=64, num_fine_samples=128, num_path_samples=12, white_bkgd=False, bg_weight=0.025, bg_smooth_weight=1.0,
                            bg_patch_size=128, use_online_sparsity=False, randomized=True, near=0.2, far=1.2, batch_size=B, config="dolphin")
    model, variables = models.construct_nerf(np.array([0, 4], np.uint32), None, flags, [G] * 3, nmin, nmax, grid)
    del grid
    pf = syn.init_params_flat(41, fine=True, bias_scale=0.05)
    for k in ("coarse_mlp", "fine_mlp", "bkgd_mlp"):
        variables["flat"][k].copy_(torch.from_numpy(pf[k]).to(dev))
    o, v = _opencv_frame(CS._look_at([c[0] + 0.45, c[1] - 0.5, c[2] + 0.2], c), 128, 128, [[187.0, 0.0, 63.3], [0.0, 188.0, 64.9], [0.0, 0.0, 1.0]], dev)
    gen = np.random.default_rng(9)
    idx = torch.from_numpy(gen.choice(128 * 128, B, replace=False)).to(dev)
    ev = gen.standard_normal((128, 128, 3)).astype(np.float32)
    ev /= np.linalg.norm(ev, axis=-1, keepdims=True)
    batch = {"rays": Rays(o[idx].contiguous(), None, v[idx].contiguous(), None),
             "pixels": torch.from_numpy(gen.uniform(0, 1, (B, 3)).astype(np.float32)).to(dev), "annealed_alpha": 0.5,
             "env_rays": Rays(None, None, torch.from_numpy(ev).to(dev), None)}
    return model, variables, flags, batch, pf


@pytest.mark.parametrize("Bd", [4096, 512])
def test_config4_dolphin_train_step_full_size(Bd):
    """Config 4 as written: hierarchical 64 + 128 train step, OpenCV rays, near 0.2 / far 1.2, G = 256, the shipped loss terms, at 4096 rays
    (global batch) and 512 rays (one of 8 GPUs).  Forward of 16 rays and the loss against the oracle; the gradient against a central
    finite difference of the device loss along the gradient direction (a checksum of the whole backward at full size)."""
    from samplenerfro_amd.train import TrainState, train_step
    from samplenerfro_amd.utils import Rays
    dev = torch.device("cuda:0")
    model, variables, flags, batch, pf = _dolphin_world(Bd, dev)
    state = TrainState.create(model, variables, flags)
    theta0 = state.theta.clone()
    rng = np.array([4, 4], np.uint32)
    taps, ftaps = {}, {}
    state.lr_fn = lambda count: 0.0                                      # keep theta: the step is evaluated three times below
    _, stats, _ = train_step(model, rng, state, batch, flags, taps=taps, forward_taps=ftaps)
    g = taps["grads"].double()
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    # --- forward parity of a ray sample (randomized resampling: u from the device threefry)
    sel = torch.arange(0, Bd, Bd // 16, device=dev)[:16]
    u = ftaps["u"][:, sel].T.cpu().numpy()
    oret, otaps = _oracle_sample(model, pf, batch["rays"].origins, batch["rays"].viewdirs, ftaps["jitter"], sel, {}, u=u)
    didx = np.abs(ftaps["idx_f"][:, sel].cpu().numpy().T.astype(np.int64) - otaps["idx_f"])
    assert didx.max() <= 1 and (didx > 0).mean() < 2e-3          # end to end: the coarse weights carry the MLP's 1e-7-level differences
    # (the forward outputs of the step are not returned by train_step: evaluate the model again with the same keys)
    from samplenerfro_amd import prng
    _, key_0, key_1 = prng.split(rng, 3)
    ret, _ = model.apply(state.variables, key_0, key_1, batch["rays"], True, 0.5)
    for lvl in range(2):
        for got, want in zip(ret[lvl][:3], oret[lvl][:3]):
            assert float(np.abs(got[sel].cpu().numpy() - want).max()) < 1e-4
    mse_f = float(((ret[1][0] - batch["pixels"]) ** 2).mean()); mse_c = float(((ret[0][0] - batch["pixels"]) ** 2).mean())
    assert abs(float(stats.loss) - mse_f) < 1e-6 and abs(float(stats.loss_c) - mse_c) < 1e-6
    # --- directional finite differences of the device loss.  The resampled fine rows depend on the COARSE parameters only, and that
    #     dependence carries no gradient (stop_gradient, model_utils.py:406-411), so: (1) along the fine + bkgd part of the gradient the
    #     total loss is differentiated (rows fixed: jitter and u are functions of the key); (2) along the coarse part only loss_c, the
    #     one term through which the coarse parameters receive gradient.
    n_theta = state.theta.numel()
    lo_c, hi_c = state.segments["coarse_mlp"]
    gt = g[:n_theta].clone()
    d1 = gt.clone(); d1[lo_c:hi_c] = 0
    d2 = torch.zeros_like(gt); d2[lo_c:hi_c] = gt[lo_c:hi_c]
    eps = 2e-3

    def loss_at(dirn, sign, which):
        state.theta.copy_(theta0 + (sign * eps * dirn).float())
        _, st, _ = train_step(model, rng, state, batch, flags)
        if which == "coarse":
            return float(st.loss_c.double())
        return float(st.loss.double() + st.loss_c.double() + st.loss_bg.double() + flags.bg_smooth_weight * st.loss_bg_smooth.double())
    for dirn, which in ((d1 / d1.norm(), "total"), (d2 / d2.norm(), "coarse")):
        fd = (loss_at(dirn, +1, which) - loss_at(dirn, -1, which)) / (2 * eps)
        analytic = float((gt * dirn).sum())
        print(f"[B={Bd}] d {which} loss along its gradient: analytic {analytic:.6e}, finite difference {fd:.6e}")
        assert abs(fd - analytic) < 0.03 * abs(analytic) + 1e-5
    state.theta.copy_(theta0)


def test_config3_ship_refractive_full_size_sample():
    """BASELINE config 3 at its full size: 4096 rays x (128 + 256) samples, N = 1536, the 512^3 sphere grid AFTER the (9, 3.0) Gaussian
    prefilter built on the device (G1 at scale: its time is recorded), the speculative march on rays that bend.  16 rays of the batch
    against the oracle on the device-built table: path / directions / depths and the resample node indices bit for bit, RGB / depth /
    opacity of both levels within 1e-4; the prefilter itself against the fp64 oracle on a 24^3 window cut out of the 512^3 grid."""
    import time
    from oracle import ref_np as R
    from samplenerfro_amd import models, ops
    from samplenerfro_amd.utils import Rays
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS["ship_refractive"]
    ext, ksize, ksigma = cfg["extent"], cfg["ksize"], cfg["ksigma"]
    a = torch.linspace(-ext, ext, G, dtype=torch.float64, device=dev)
    r = torch.sqrt(a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2)
    raw = (((1.0 + 0.33 * torch.clamp((cfg["radius"] - r) / (2.0 * ext / (G - 1)) + 0.5, 0.0, 1.0)) - 1.0) * cfg["ri"] / 0.33 + 1.0).float()
    del r
    ops.grid_prefilter(raw[:64, :64, :64].contiguous(), ksize, ksigma)                   # (first call: module load)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    grid = ops.grid_prefilter(raw, ksize, ksigma)
    torch.cuda.synchronize()
    t_pref = time.perf_counter() - t0
    print(f"rnerf_grid_prefilter (9, 3.0) at 512^3: {1e3 * t_pref:.1f} ms (3 separable passes, 0.54 GB in + out each)")
    assert t_pref < 0.5
    # G1 at scale: a window around the sphere's boundary (where the grid is not constant) against the dense fp64 kernel of the reference
    lo = G // 2 + int(0.6 / (2 * ext / (G - 1))) - 12                                    # the boundary crosses the window along x
    w0, w1 = lo - 4, lo + 24 + 4                                                         # + the kernel's halo
    win = raw[w0:w1, G // 2 - 16:G // 2 + 16, G // 2 - 16:G // 2 + 16].double().cpu().numpy()
    want = R.conv3d_normal(win.reshape(-1, 1), list(win.shape), ksize, ksigma, dtype=np.float64).reshape(win.shape)[4:-4, 4:-4, 4:-4]
    got = grid[w0 + 4:w1 - 4, G // 2 - 12:G // 2 + 12, G // 2 - 12:G // 2 + 12].cpu().numpy()
    assert float(np.abs(want).max()) > 1.2 and float(np.ptp(want)) > 0.2                 # the window really holds the boundary
    assert float(np.abs(got - want).max()) < 2e-6
    del raw
    model = models.NerfModel(ndim=[G] * 3, nmin=[-ext] * 3, nmax=[ext] * 3, grid=grid, near=cfg["near"], far=cfg["far"], num_coarse_samples=S,
                             num_fine_samples=256, num_path_samples=P, device=dev)
    del grid
    pf = syn.init_params_flat(0, fine=True, bias_scale=0.05)
    variables = models.make_variables({k: torch.from_numpy(v).to(dev) for k, v in pf.items()})
    o, d = syn.sphere_rays(B)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    key = np.array([0, 3], np.uint32)
    taps = {}
    ret, _ = model.apply(variables, key, key, Rays(o, None, d, None), False, taps=taps)
    n_path = taps["path_ior"][..., 0]
    bent = (n_path.max(0).values > 1.4)
    assert int(bent.sum()) > 500                                                         # a good part of the batch crosses the sphere
    # 16 rays: 12 that cross the refractive sphere, 4 that miss it
    idx_b = torch.nonzero(bent).reshape(-1)
    idx_m = torch.nonzero(~bent).reshape(-1)
    sel = torch.cat([idx_b[:: max(len(idx_b) // 12, 1)][:12], idx_m[:: max(len(idx_m) // 4, 1)][:4]])
    oret, otaps = _oracle_sample(model, pf, o, d, taps["jitter"], sel, {})
    pd = taps["path_pd"][:, sel].cpu().numpy()
    assert np.array_equal(pd[..., :3].transpose(1, 0, 2), otaps["ray_pos"]) and np.array_equal(pd[..., 3].T, otaps["ray_dist"])
    assert np.array_equal(taps["path_dr"][:, sel].cpu().numpy()[..., :3].transpose(1, 0, 2), otaps["ray_dir"])
    # resample node indices: bit-exact GIVEN the same coarse weights (the oracle's sample_pdf fed the device's weights); end to end the
    # weights differ by the MLP's ~1e-7, which may move a fine depth across a node depth for a few samples in ten thousand
    gi = taps["idx_f"][:, sel].cpu().numpy().T
    w_dev = taps["weights_c"][:, sel].cpu().numpy().T
    jit = np.asarray(taps["jitter"], np.int64)
    t_c = otaps["ray_dist"][:, jit]
    mid = np.float32(0.5) * (t_c[..., 1:] + t_c[..., :-1])
    _, _, _, _, idx_o = R.sample_pdf(R.linspace_u(256, len(sel), np.float32), mid, w_dev[..., 1:-1], otaps["ray_pos"], otaps["ray_dir"], otaps["ray_dist"],
                                     otaps["idx_grad"], jit)
    assert np.array_equal(gi, idx_o)
    assert float((gi != otaps["idx_f"]).mean()) < 2e-3
    for lvl in range(2):
        for got_t, want_a in zip(ret[lvl][:3], oret[lvl][:3]):
            assert float(np.abs(got_t[sel].cpu().numpy() - want_a).max()) < 1e-4
    # whole-path call (rnerf_forward) on the full batch = the staged sequence with taps, bit for bit
    ret_w, _ = model.apply(variables, key, key, Rays(o, None, d, None), False)
    for la, lb in zip(ret_w, ret):
        for x, y in zip(la, lb):
            assert torch.equal(x, y)


def test_march_coresident_with_the_wgrad_changes_no_bit(world):
    """The product train step at bench size (4096 x 128 flat, 512^3): the next batch's march is forked right before the NerfMLP wgrad and
    runs co-resident with it on every CU (rnerf_prefetch; the wgrad is held to 224 registers for that).  Sharing SIMDs must
    change nothing: the prefetched path record equals a stand-alone march of the same rays bit for bit, and the step's gradient equals the
    gradient of the same step issued without any prefetch."""
    from samplenerfro_amd import ops, utils
    from samplenerfro_amd.train import TrainState, train_step
    from samplenerfro_amd.utils import Rays
    import copy
    dev = torch.device("cuda:0")
    m = copy.copy(world["sphere"])
    m.num_fine_samples = 0
    m._packed, m._jit_cache, m._ws, m._key_cache, m._u_lin, m._side, m._tail = {}, {}, {}, {}, None, None, None
    pf = syn.init_params_flat(0, fine=False, bias_scale=0.05)
    from samplenerfro_amd import models
    flags = utils.default_flags(num_coarse_samples=S, num_fine_samples=0, num_path_samples=P, white_bkgd=False, bg_weight=0.025, bg_smooth_weight=1.0,
                                bg_patch_size=128, use_online_sparsity=False, randomized=True, near=m.near, far=m.far)
    rng = np.random.default_rng(11)
    pix = torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32)).to(dev)
    ev = rng.standard_normal((128, 128, 3)).astype(np.float32); ev /= np.linalg.norm(ev, axis=-1, keepdims=True)
    o2, d2 = syn.sphere_rays(B, seed=99)
    nxt = Rays(torch.from_numpy(o2).to(dev), None, torch.from_numpy(d2).to(dev), None)
    batch = {"rays": world["rays"], "pixels": pix, "annealed_alpha": 0.5, "env_rays": Rays(None, None, torch.from_numpy(ev).to(dev), None)}
    grads = []
    for prefetch in (True, False):
        variables = models.make_variables({k: torch.from_numpy(v).to(dev) for k, v in pf.items()})
        state = TrainState.create(m, variables, flags)
        state, stats, _ = train_step(m, np.array([5, 6], np.uint32), state, batch, flags, next_rays=nxt if prefetch else None)
        torch.cuda.synchronize()
        grads.append(state.grads[:state.theta.numel()].clone())
        assert bool(torch.isfinite(stats.loss))
        if prefetch:
            h = state.next_path
            h.event.synchronize()
            pd, dr, _, _ = ops.march(m.table, m.spec, nxt.origins, nxt.viewdirs, m.near, m.far, N)
            assert torch.equal(h.pd, pd) and torch.equal(h.dr, dr)
    assert torch.equal(grads[0], grads[1])


def test_bricked_table_at_full_size_renders_the_same_bits():
    """BASELINE configs[2] at full size (4096 rays x (128 + 256) samples, N = 1536, 512^3 table after the (9, 3.0) prefilter) with the IoR
    table in 2x2x2 bricks (include/rnerf.h: rnerf_table_layout) against the reference order: path, both levels' outputs — every bit."""
    from samplenerfro_amd import models, ops, prng, synthetic as syn
    from samplenerfro_amd.utils import Rays
    dev = torch.device("cuda:0")
    cfg = dict(syn.CONFIGS["ship_refractive"])
    G, ext = cfg["G"], cfg["extent"]
    a = torch.linspace(-ext, ext, G, dtype=torch.float64, device=dev)
    r = torch.sqrt(a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2)
    h = 2.0 * ext / (G - 1)
    grid = ((0.33 * torch.clamp((cfg["radius"] - r) / h + 0.5, 0.0, 1.0)) * cfg["ri"] / 0.33 + 1.0).float()
    del r
    grid = ops.grid_prefilter(grid, cfg["ksize"], cfg["ksigma"])
    pf = syn.init_params_flat(0, fine=True)
    o, d = syn.sphere_rays(4096, seed=syn.SEED)
    rays = Rays(torch.from_numpy(o).to(dev), None, torch.from_numpy(d).to(dev), None)
    key = prng.PRNGKey(3)
    outs, paths = {}, {}
    for layout in ("reference", "bricks"):
        m = models.NerfModel(ndim=[G] * 3, nmin=[-ext] * 3, nmax=[ext] * 3, grid=grid, near=cfg["near"], far=cfg["far"], num_coarse_samples=cfg["S"],
                             num_fine_samples=256, num_path_samples=cfg["P"], table_layout=layout, device=dev)
        v = models.make_variables({k: torch.from_numpy(x).to(dev) for k, x in pf.items()})
        paths[layout] = ops.march(m.table, m.spec, rays.origins, rays.viewdirs, m.near, m.far, m.num_samples)[:2]
        outs[layout], _ = m.apply(v, key, key, rays, True)
        del m
        torch.cuda.empty_cache()
    bent = (paths["reference"][1][-1, :, :3] - paths["reference"][1][0, :, :3]).abs().max()
    assert float(bent) > 1e-3                                     # rays do bend through the sphere
    for a_, b_ in zip(paths["reference"], paths["bricks"]):
        assert torch.equal(a_, b_)
    for lvl in range(2):
        for a_, b_ in zip(outs["reference"][lvl], outs["bricks"][lvl]):
            assert torch.equal(a_, b_)

