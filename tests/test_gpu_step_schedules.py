"""The three backward schedules of rnerf_train_forward_backward (csrc/pipeline.hip: one stream; aux stream with the levels in sequence;
aux stream with the levels side by side) and the workspace carve they share with rnerf_forward.

The grads_stream test is a tripwire for a fork placed ahead of the last wgrad, not a proof of the issue order: that is the trace
comparison of profiles/step_schedules/."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step_dump():
    spec = importlib.util.spec_from_file_location("step_dump", os.path.join(ROOT, "tools", "step_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("Nf,B,aux", [(0, 160, False), (24, 160, False), (0, 160, True), (24, 2500, True), (24, 160, True)],
                         ids=["one_stream_flat", "one_stream_hierarchical", "aux_flat", "aux_levels_in_sequence", "aux_levels_side_by_side"])
def test_grads_stream_is_forked_behind_the_last_wgrad(Nf, B, aux, monkeypatch):
    """rnerf_train_cfg.grads_stream: when rnerf_train_forward_backward returns, that stream is ordered behind the last NerfMLP wgrad —
    a copy of the NerfMLP gradient segments enqueued on it right away holds what `stream` itself sees once the call's work is done."""
    from samplenerfro_amd import _lib, train
    model, variables, batch, flags = _step_dump()._scene(Nf, B, None)
    state = train.TrainState.create(model, variables, flags)
    side = torch.cuda.Stream()
    real_cfg = train.train_cfg

    def cfg(model, state, flags, annealed):
        c = real_cfg(model, state, flags, annealed)
        if not aux:
            c.aux_stream = None
        c.grads_stream = side.cuda_stream
        return c
    monkeypatch.setattr(train, "train_cfg", cfg)
    lib = _lib.load()
    real_call = lib.rnerf_train_forward_backward
    n_big = state.segments["bkgd_mlp"][0]
    got = {}

    def call(*args):
        rc = real_call(*args)
        with torch.cuda.stream(side):
            got["side"] = state.grads[:n_big].clone()
        got["main"] = state.grads[:n_big].clone()        # behind everything the call enqueued or joined, ahead of the optimiser's clip
        return rc
    monkeypatch.setattr(lib, "rnerf_train_forward_backward", call)
    train.train_step(model, np.array([1, 2], np.uint32), state, batch, flags)
    torch.cuda.synchronize()
    assert n_big == 595844 * (2 if Nf > 0 else 1)
    assert torch.equal(got["side"].view(torch.int32), got["main"].view(torch.int32))
    for lo in range(0, n_big, 595844):                   # every level's segment was written
        assert float(got["main"][lo:lo + 595844].abs().max()) > 0


# (entry, Nc, Nf, P, B, bd_cut, patch, aux, backward) -> bytes: the parent commit's answers, recorded on the MI355X (256 CUs)
WORKSPACE_BYTES = [
    (("fwd", 16, 0, 4, 160, 0, 0, 0, "f16x3"), 383488),
    (("fwd", 16, 24, 4, 160, 1, 0, 0, "f16x3"), 743424),
    (("train", 16, 0, 4, 160, 0, 8, 1, "f16x3"), 289912576),
    (("train", 16, 0, 4, 2500, 0, 0, 0, "bf16"), 668912896),
    (("train", 16, 24, 4, 160, 0, 8, 0, "f16x3"), 401520640),
    (("train", 16, 24, 4, 160, 0, 8, 1, "f16x3"), 656110080),          # levels side by side: the coarse level's own dY / d raw / wgrad scratch
    (("train", 16, 24, 4, 2500, 1, 8, 1, "f16x3"), 2711102464),        # levels in sequence
    (("train", 64, 128, 4, 160, 1, 0, 0, "bf16"), 617500672),
]


def test_workspace_sizes_are_the_parents():
    from samplenerfro_amd import _lib
    lib = _lib.load()
    for (entry, Nc, Nf, P, B, bd, patch, aux, bwd), want in WORKSPACE_BYTES:
        m = _lib.Model()
        m.table, m.num_coarse, m.num_fine, m.num_path, m.bd_cut, m.precision = 256, Nc, Nf, P, bd, _lib.PREC_F16X3
        if entry == "fwd":
            got = lib.rnerf_forward_workspace_bytes(C.byref(m), B)
        else:
            c = _lib.TrainCfg()
            c.backward, c.bg_patch_size, c.bg_smooth_weight, c.aux_stream = _lib.BACKWARDS[bwd], patch, 1.0 if patch else 0.0, 256 if aux else None
            got = lib.rnerf_train_workspace_bytes(C.byref(m), C.byref(c), B)
        assert got == want, (entry, Nc, Nf, P, B, bd, patch, aux, bwd)
