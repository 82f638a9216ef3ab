"""The serial small-kernel chain of the training step: the two-launch optimiser (rnerf_adam_update_fused) must give the bits of the
three-kernel sequence (rnerf_adam_update, kept as the reference), and moving the background-MLP backward + the statistics to the aux
stream, beside the last NerfMLP wgrad, must change the order of execution only."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"
N_THETA = 595844 + 56963        # the flat model of the bench: one NerfMLP + the background MLP
N_FROZEN = 65411                # the frozen so3 MLP


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _adam_cfg(_lib, wd, gv, gn, skip):
    a = _lib.AdamCfg()
    a.lr_init, a.lr_final, a.lr_delay_mult, a.max_steps, a.lr_delay_steps = 5e-4, 5e-6, 0.01, 200000, 2500
    a.b1, a.b2, a.eps, a.weight_decay_mult, a.grad_max_val, a.grad_max_norm = 0.9, 0.999, 1e-8, wd, gv, gn
    a.n_all, a.lr_override, a.use_lr_override, a.skip_nonfinite = N_THETA + N_FROZEN, 0.0, 0, skip
    return a


@pytest.mark.parametrize("name,wd,gv,gn,frozen,bad,skip", [
    ("plain", 0.0, 0.0, 0.0, False, False, 1),
    ("value_clip", 0.0, 0.02, 0.0, False, False, 1),
    ("norm_clip", 0.0, 0.0, 0.5, False, False, 1),
    ("decay_frozen", 3.0, 0.02, 0.5, True, False, 1),
    ("nonfinite_skip_on", 3.0, 0.02, 0.5, True, True, 1),
    ("nonfinite_skip_off", 3.0, 0.02, 0.5, True, True, 0),
])
def test_fused_optimiser_equals_the_three_kernel_sequence(name, wd, gv, gn, frozen, bad, skip):
    """theta, mu, nu, grads, scratch[0..3] and the step counter of rnerf_adam_update_fused against rnerf_adam_update on random buffers of the
    bench's size, bit for bit; the word written to pinned host memory is scratch[3]."""
    from samplenerfro_amd import _lib
    lib = _lib.load()
    g = np.random.default_rng(11)
    theta = g.standard_normal(N_THETA).astype(F32); mu = (0.01 * g.standard_normal(N_THETA)).astype(F32)
    nu = (1e-4 * g.random(N_THETA)).astype(F32); grads = (0.05 * g.standard_normal(N_THETA + 8)).astype(F32)
    fr = g.standard_normal(N_FROZEN).astype(F32)
    if bad:
        grads[12345] = np.nan; grads[N_THETA - 7] = np.inf
    out = {}
    for fused in (False, True):
        a = _adam_cfg(_lib, wd, gv, gn, skip)
        t_th, t_mu, t_nu, t_g, t_fr = T(theta), T(mu), T(nu), T(grads), T(fr)
        step = torch.tensor([2499], dtype=torch.int32, device=DEV)
        scratch = torch.full((_lib.ADAM_SCRATCH_FLOATS,), -7.0, device=DEV)       # no initial contents needed
        word = torch.full((1,), -1.0).pin_memory()
        args = (C.byref(a), t_th.data_ptr(), t_mu.data_ptr(), t_nu.data_ptr(), t_g.data_ptr(), N_THETA, t_fr.data_ptr() if frozen else None,
                N_FROZEN if frozen else 0, step.data_ptr(), scratch.data_ptr())
        if fused:
            _lib.check(lib.rnerf_adam_update_fused(*args, word.data_ptr(), _lib.current_stream()), "rnerf_adam_update_fused")
        else:
            _lib.check(lib.rnerf_adam_update(*args, _lib.current_stream()), "rnerf_adam_update")
        torch.cuda.synchronize()
        if fused:
            assert float(word[0]) == float(scratch[3])
        out[fused] = (_bits(t_th), _bits(t_mu), _bits(t_nu), _bits(t_g), _bits(scratch[:4]), int(step.item()), float(scratch[3]))
    for i, what in enumerate(("theta", "mu", "nu", "grads", "scal")):
        assert torch.equal(out[True][i], out[False][i]), (name, what)
    assert out[True][5] == out[False][5] == 2500
    assert out[True][6] == (2.0 if bad else 0.0)
    if bad and skip:        # nothing moved
        assert torch.equal(out[True][0], _bits(T(theta))) and torch.equal(out[True][1], _bits(T(mu))) and torch.equal(out[True][2], _bits(T(nu)))
    else:
        assert not torch.equal(out[True][0], _bits(T(theta)))


def test_fused_optimiser_without_a_partials_launch_keeps_the_old_sequence():
    """No decay, no clip, no skip: there is no prep launch, adam_apply counts the non-finite entries itself; same bits, word included."""
    from samplenerfro_amd import _lib
    lib = _lib.load()
    g = np.random.default_rng(5)
    n = 100003
    theta = g.standard_normal(n).astype(F32); grads = (0.05 * g.standard_normal(n)).astype(F32); grads[17] = np.inf
    out = {}
    for fused in (False, True):
        a = _adam_cfg(_lib, 0.0, 0.0, 0.0, 0); a.n_all = n
        t_th, t_mu, t_nu, t_g = T(theta), T(np.zeros(n, F32)), T(np.zeros(n, F32)), T(grads)
        step = torch.tensor([3], dtype=torch.int32, device=DEV)
        scratch = torch.zeros(_lib.ADAM_SCRATCH_FLOATS, device=DEV)
        word = torch.full((1,), -1.0).pin_memory()
        args = (C.byref(a), t_th.data_ptr(), t_mu.data_ptr(), t_nu.data_ptr(), t_g.data_ptr(), n, None, 0, step.data_ptr(), scratch.data_ptr())
        if fused:
            _lib.check(lib.rnerf_adam_update_fused(*args, word.data_ptr(), _lib.current_stream()), "rnerf_adam_update_fused")
        else:
            _lib.check(lib.rnerf_adam_update(*args, _lib.current_stream()), "rnerf_adam_update")
        torch.cuda.synchronize()
        if fused:
            assert float(word[0]) == float(scratch[3]) == 1.0
        out[fused] = (_bits(t_th), _bits(t_mu), _bits(t_nu), _bits(scratch[:4]), int(step.item()))
    for i in range(4):
        assert torch.equal(out[True][i], out[False][i])
    assert out[True][4] == out[False][4] == 4


def _train_setup(Nf, B):
    from oracle import ref_np as R
    from samplenerfro_amd import models, synthetic as syn, utils
    from samplenerfro_amd.train import TrainState
    G = 24
    ndim, nmin, nmax = [G] * 3, [-1.5] * 3, [1.5] * 3
    grid = R.conv3d_normal(syn.scale_ior(syn.sphere_grid(G, 1.5, 0.6), 0.5).reshape(-1, 1), ndim, 3, 1.0).reshape(ndim)
    model = models.NerfModel(ndim=ndim, nmin=nmin, nmax=nmax, grid=T(grid.astype(F32)), num_coarse_samples=16, num_fine_samples=Nf,
                             num_path_samples=4, precision="f16x3", white_bkgd=False)
    pf = syn.init_params_flat(3, fine=Nf > 0, bias_scale=0.1)
    variables = models.make_variables({k: T(v) for k, v in pf.items()})
    o, d = syn.sphere_rays(B, seed=3)
    rays = utils.Rays(T(o), None, T(d), None)
    flags = utils.default_flags(num_coarse_samples=16, num_fine_samples=Nf, num_path_samples=4, white_bkgd=False, bg_weight=0.025, bg_smooth_weight=1.0,
                                bg_patch_size=8, use_online_sparsity=False, randomized=True, lr_delay_steps=10, max_steps=1000)
    rng = np.random.default_rng(7)
    ev = rng.standard_normal((8, 8, 3)).astype(F32); ev /= np.linalg.norm(ev, axis=-1, keepdims=True)
    batch = {"rays": rays, "pixels": T(rng.uniform(0, 1, (B, 3)).astype(F32)), "annealed_alpha": 0.5, "env_rays": utils.Rays(None, None, T(ev), None)}
    return model, TrainState.create(model, variables, flags), batch, flags


@pytest.mark.parametrize("Nf,B", [(0, 160), (0, 1000), (24, 160), (24, 2500)])
def test_train_step_with_and_without_an_aux_stream_gives_the_same_bits(Nf, B, monkeypatch):
    """With an aux stream the background-MLP backward, the env-map term and the statistics run beside the last NerfMLP wgrad, without one
    behind it: every gradient segment, the eight statistics and the updated parameters must be the same bits (flat model, and a hierarchical
    one both with its levels side by side — 160 rays — and one after the other — 2500 rays), step after step."""
    from samplenerfro_amd import train
    real_cfg = train.train_cfg
    out = {}
    for with_aux in (True, False):
        def cfg(model, state, flags, annealed, _aux=with_aux):
            c = real_cfg(model, state, flags, annealed)
            if not _aux:
                c.aux_stream = None
            return c
        monkeypatch.setattr(train, "train_cfg", cfg)
        model, state, batch, flags = _train_setup(Nf, B)
        rng = np.array([1, 2], np.uint32)
        got = []
        for _ in range(2):
            state, stats, rng = train.train_step(model, rng, state, batch, flags)
            torch.cuda.synchronize()
            got.append((_bits(state.grads), _bits(state.theta), _bits(state.mu), _bits(state.nu)))
        out[with_aux] = got
    for a, b in zip(out[True], out[False]):
        for x, y, what in zip(a, b, ("grads + stats8", "theta", "mu", "nu")):
            assert torch.equal(x, y), what
    assert float(out[True][0][0].view(torch.float32)[:-8].abs().max()) > 0


def test_lagged_range_retry_reads_the_word_the_update_wrote():
    """range_retry="lag": the non-finite count reaches the pinned host word from the update's own launch (no copy launch behind the step)."""
    from samplenerfro_amd import train
    model, state, batch, flags = _train_setup(0, 160)
    assert flags.range_retry == "lag"
    state._lag_host.fill_(-1.0)
    rng = np.array([1, 2], np.uint32)
    for i in range(3):
        state, stats, rng = train.train_step(model, rng, state, batch, flags)
        torch.cuda.synchronize()
        assert float(state._lag_host[i]) == float(state.adam_scratch[3]) == 0.0
    train.flush_range_retry(model, state)
    assert state.step == 3 and state.range_retries == 0
