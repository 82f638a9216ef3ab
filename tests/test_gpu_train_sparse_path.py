"""The flat train step's prefetched path is sparse: the march of step k + 1, issued in step k, draws step k + 1's jitter (from the keys
step k derives one step ahead) and records only its nodes; step k + 1 reads the path through that very array.  Three pipelined steps on a
tiny flat model (64 rays x 8 samples, P = 4, a 16^3 table), every slot buffer poisoned with NaN before its march, against the same three
steps without any handle: parameters, both Adam moments, the gradient buffer and every Stats field, bit for bit.  A handle whose key is
not the step's is not used; hierarchical models and stage "all" get no sparse handle; a dense consumer refuses a sparse one."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"
B, S, P, G, STEPS = 64, 8, 4, 16, 3


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _setup(Nf=0):
    from oracle import ref_np as R
    from samplenerfro_amd import models, synthetic as syn, utils
    from samplenerfro_amd.train import TrainState
    ndim, nmin, nmax = [G] * 3, [-1.5] * 3, [1.5] * 3
    grid = R.conv3d_normal(syn.scale_ior(syn.sphere_grid(G, 1.5, 0.6), 0.5).reshape(-1, 1), ndim, 3, 1.0).reshape(ndim)
    model = models.NerfModel(ndim=ndim, nmin=nmin, nmax=nmax, grid=T(grid.astype(F32)), num_coarse_samples=S, num_fine_samples=Nf,
                             num_path_samples=P, precision="f16x3", white_bkgd=False)
    pf = syn.init_params_flat(3, fine=Nf > 0, bias_scale=0.1)
    variables = models.make_variables({k: T(v) for k, v in pf.items()})
    flags = utils.default_flags(num_coarse_samples=S, num_fine_samples=Nf, num_path_samples=P, white_bkgd=False, bg_weight=0.025, bg_smooth_weight=1.0,
                                bg_patch_size=8, use_online_sparsity=False, randomized=True, lr_delay_steps=10, max_steps=1000)
    gen = np.random.default_rng(7)
    ev = gen.standard_normal((8, 8, 3)).astype(F32); ev /= np.linalg.norm(ev, axis=-1, keepdims=True)
    env = utils.Rays(None, None, T(ev), None)
    batches = []
    for k in range(STEPS + 1):
        o, d = syn.sphere_rays(B, seed=20 + k)
        batches.append({"rays": utils.Rays(T(o), None, T(d), None), "pixels": T(gen.uniform(0, 1, (B, 3)).astype(F32)), "annealed_alpha": 0.5,
                        "env_rays": env})
    return model, TrainState.create(model, variables, flags), batches, flags


def _poison_slots(model, handles):
    """Every slot buffer prefetch_slot hands out is filled with NaN (on the step's stream, i.e. before the march that is forked from it)."""
    inner = model.prefetch_slot

    def prefetch_slot(rays, **kw):
        h, nxt = inner(rays, **kw)
        for t in h.raw():
            t.fill_(float("nan"))
        handles.append(h)
        return h, nxt
    model.prefetch_slot = prefetch_slot


def _snapshot(state, stats):
    out = {"theta": state.theta.clone(), "mu": state.mu.clone(), "nu": state.nu.clone(), "grads": state.grads.clone()}
    for f in dataclasses.fields(stats):
        v = getattr(stats, f.name)
        out["stats_" + f.name] = v.clone() if isinstance(v, torch.Tensor) else torch.tensor(float(v))
    return out


def _run(pipelined, reseed_at=None, spoil=False):
    """STEPS train steps; pipelined: each step marches the next batch (next_rays) and the next step gets the handle.  reseed_at: that step
    is called with an rng of the caller's own instead of the one the step before returned.  spoil: every record of a handle that must not
    be used is overwritten with NaN first."""
    from samplenerfro_amd.train import flush_range_retry, train_step
    model, state, batches, flags = _setup()
    handles = []
    if pipelined:
        _poison_slots(model, handles)
    rng = np.array([1, 2], np.uint32)
    snaps, path = [], None
    for k in range(STEPS):
        if reseed_at == k:
            rng = np.array([77, 78], np.uint32)
            if spoil and path is not None:
                path.event.synchronize()
                for t in path.raw():
                    t.fill_(float("nan"))
        _, stats, rng = train_step(model, rng, state, batches[k], flags, path=path, next_rays=batches[k + 1]["rays"] if pipelined else None)
        path = state.next_path if pipelined else None
        snaps.append(_snapshot(state, stats))
    flush_range_retry(model, state)
    torch.cuda.synchronize()
    return snaps, handles, model, state


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for name in x:
            assert torch.equal(x[name].view(torch.int32), y[name].view(torch.int32)), (k, name)
        assert bool(torch.isfinite(x["theta"]).all()) and bool(torch.isfinite(x["stats_loss"]))


@pytest.fixture(scope="module")
def plain():
    return _run(False)[0]


def test_three_pipelined_steps_on_sparse_paths_equal_the_steps_without_a_handle(plain):
    from samplenerfro_amd import prng
    snaps, handles, model, state = _run(True)
    _same(snaps, plain)
    # the handles were sparse, drawn from the keys of the step they were for, and the march wrote the sampled nodes only
    assert len(handles) == STEPS
    rng = np.array([1, 2], np.uint32)
    for h in handles:
        rng, _, _ = prng.step_keys(rng)
        key_0 = prng.step_keys(rng)[1]
        assert h.sparse and h.matches(key_0)
        jit = prng.step_jitter(key_0, S, P, model.use_random_choice)
        assert np.array_equal(h.jitter.cpu().numpy(), jit)
        sampled = np.zeros(S * P, bool); sampled[jit] = True
        pd, dr = (t.cpu().numpy() for t in h.raw())
        assert np.isfinite(pd[sampled]).all() and np.isfinite(dr[sampled]).all()
        assert np.isnan(pd[~sampled]).all() and np.isnan(dr[~sampled]).all()


def test_a_handle_drawn_from_another_key_is_not_used(plain):
    """The caller re-seeds before step 1: the handle step 0 left was drawn from the key step 0 expected.  Its records are all NaN here, so
    any use of it would show; the steps equal the same (re-seeded) sequence without handles."""
    want = _run(False, reseed_at=1)[0]
    got, handles, _, _ = _run(True, reseed_at=1, spoil=True)
    _same(got, want)
    assert any(not torch.equal(a["theta"], b["theta"]) for a, b in zip(want[1:], plain[1:]))      # (the re-seeding did change the steps)


def test_hierarchical_models_get_dense_handles():
    from samplenerfro_amd import ops
    from samplenerfro_amd.train import train_step
    model, state, batches, flags = _setup(Nf=8)
    train_step(model, np.array([1, 2], np.uint32), state, batches[0], flags, next_rays=batches[1]["rays"])
    h = state.next_path
    h.event.synchronize()
    assert not h.sparse and h.jitter is None
    r = batches[1]["rays"]
    pd, dr, _, _ = ops.march(model.table, model.spec, r.origins, r.viewdirs, model.near, model.far, S * P)
    assert torch.equal(h.pd, pd) and torch.equal(h.dr, dr)
    with pytest.raises(ValueError):
        model.prefetch_slot(r, next_keys=(np.array([1, 2], np.uint32), np.array([3, 4], np.uint32)))


def test_a_stage_all_step_leaves_no_sparse_handle():
    from samplenerfro_amd import models, synthetic as syn, utils
    from samplenerfro_amd.train import TrainState, train_step
    from oracle import ref_np as R
    grid = R.conv3d_normal(syn.scale_ior(syn.sphere_grid(G, 1.5, 0.6), 0.5).reshape(-1, 1), [G] * 3, 3, 1.0).reshape(G, G, G)
    flags = utils.default_flags(stage="all", num_coarse_samples=S, num_fine_samples=0, num_path_samples=P, white_bkgd=False, bg_weight=0.025,
                                bg_smooth_weight=1.0, bg_patch_size=8, use_online_sparsity=False, lr_delay_steps=0, max_steps=1000, near=2.0, far=6.0,
                                randomized=False)
    model, variables = models.construct_nerf(np.array([0, 7], np.uint32), None, flags, [G] * 3, [-1.5] * 3, [1.5] * 3, T(grid.astype(F32)))
    gen = np.random.default_rng(5)
    o, d = syn.sphere_rays(B, seed=5)
    ev = gen.standard_normal((8, 8, 3)).astype(F32); ev /= np.linalg.norm(ev, axis=-1, keepdims=True)
    batch = {"rays": utils.Rays(T(o), T(d), T(d), None), "pixels": T(gen.uniform(0, 1, (B, 3)).astype(F32)), "annealed_alpha": 0.5,
             "env_rays": utils.Rays(None, None, T(ev), None)}
    state = TrainState.create(model, variables, flags)
    _, stats, _ = train_step(model, np.array([1, 2], np.uint32), state, batch, flags, next_rays=batch["rays"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(stats.loss))
    assert state.next_path is None or not state.next_path.sparse


def test_a_sparse_handle_passed_to_a_dense_consumer_raises():
    from samplenerfro_amd import prng
    from samplenerfro_amd.train import train_step
    model, state, batches, flags = _setup()
    train_step(model, np.array([1, 2], np.uint32), state, batches[0], flags, next_rays=batches[1]["rays"])
    h = state.next_path
    assert h.sparse
    k0, k1 = prng.PRNGKey(5), prng.PRNGKey(9)
    for whole in (True, False):                              # rnerf_forward in one call, and the staged sequence
        model.whole_path = whole
        with pytest.raises(ValueError, match="jitter"):
            model.apply(state.variables, k0, k1, batches[1]["rays"], False, path=h)
    torch.cuda.synchronize()


def test_reading_pd_of_a_sparse_handle_completes_the_record_and_keeps_the_prefetched_nodes():
    """handle.pd / handle.dr are the whole record, as for every handle: read on a sparse one, the nodes its march skipped are marched then
    (into the poisoned buffers here), the nodes it recorded keep the prefetch's own records, and the handle is dense from there on."""
    from samplenerfro_amd import ops
    from samplenerfro_amd.train import train_step
    model, state, batches, flags = _setup()
    handles = []
    _poison_slots(model, handles)
    train_step(model, np.array([1, 2], np.uint32), state, batches[0], flags, next_rays=batches[1]["rays"])
    h = state.next_path
    assert h is handles[0] and h.sparse
    h.event.synchronize()
    before = [t.clone() for t in h.raw()]
    at = h.jitter.long()
    r = batches[1]["rays"]
    pd, dr, _, _ = ops.march(model.table, model.spec, r.origins, r.viewdirs, model.near, model.far, S * P)
    assert torch.equal(h.pd.view(torch.int32), pd.view(torch.int32)) and torch.equal(h.dr.view(torch.int32), dr.view(torch.int32))
    assert not h.sparse
    assert torch.equal(h.pd[at].view(torch.int32), before[0][at].view(torch.int32)) and torch.equal(h.dr[at].view(torch.int32), before[1][at].view(torch.int32))
    model.whole_path = True                                  # a dense consumer takes it now
    model.apply(state.variables, np.array([5, 6], np.uint32), np.array([7, 8], np.uint32), r, False, path=h)
    torch.cuda.synchronize()
