"""Host-side mirror of rnerf/models.py: `NerfModel` and `construct_nerf` with the reference's call surface.

`model.apply(variables, rng_0, rng_1, rays, randomized, annealed_alpha)` returns `(ret, loss_sp)` exactly like
`NerfModel.__call__` (rnerf/models.py:220-535): `ret` is a list of one (N_f == 0) or two tuples
`(comp_rgb [B,3], distance [B], acc [B], trans [B,1], trans_rgb_bkgd [B,3])`, coarse first.

All arithmetic happens in librnerf.so (samplenerfro_amd/csrc); this file only sequences the stage calls and owns the
parameter tree.  There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops, prng
from ._lib import Grid, PRECISIONS
from .utils import Rays

# Dense shapes in flax creation order (rnerf/model_utils.py:58-89, :119-138; ior_utils.py:148-152)
NERF_MLP_SHAPES = [(63, 256), (256, 256), (256, 256), (256, 256), (256, 256), (319, 256), (256, 256), (256, 256),
                   (256, 1), (256, 256), (283, 128), (128, 3)]
BKGD_MLP_SHAPES = [(27, 128), (128, 128), (128, 128), (155, 128), (128, 3)]
SO3_MLP_SHAPES = [(60, 128), (128, 128), (128, 128), (188, 128), (128, 3)]


_STREAMS: Dict[Tuple[str, str], "torch.cuda.Stream"] = {}


def shared_stream(device, role: str) -> "torch.cuda.Stream":
    """ONE side stream per (device, role) for the whole process, whatever the number of models.  HIP streams are multiplexed onto a few
    hardware queues (GPU_MAX_HW_QUEUES, 4 by default), assigned in creation order: a process that gives every model its own march / tail /
    collective streams soon has two streams of ONE model on one queue, and the work they were meant to overlap runs in sequence (measured:
    a 128-ray train step 1.11 -> 1.46 ms inside the bench, which builds seven models; profiles/r04/small_batches.txt)."""
    d = torch.device(device)
    if d.index is None:                     # "cuda" and "cuda:<current>" are one device: one key
        d = torch.device("cuda", torch.cuda.current_device())
    key = (str(d), role)
    s = _STREAMS.get(key)
    if s is None:
        s = _STREAMS[key] = torch.cuda.Stream(device=d)
    return s


def flat_size(shapes) -> int:
    return sum(i * o + o for i, o in shapes)


def flat_to_tree(flat: torch.Tensor, shapes) -> Dict[str, Dict[str, torch.Tensor]]:
    """Views of a flat fp32 buffer as the flax tree {Dense_k: {kernel [in,out], bias [out]}} (SURVEY.md §5 checkpoint)."""
    tree, off = {}, 0
    for k, (i, o) in enumerate(shapes):
        tree[f"Dense_{k}"] = {"kernel": flat[off:off + i * o].view(i, o), "bias": flat[off + i * o:off + i * o + o]}
        off += i * o + o
    assert off == flat.numel()
    return tree


def tree_to_flat(tree, shapes, device=None) -> torch.Tensor:
    parts = []
    for k, (i, o) in enumerate(shapes):
        d = tree[f"Dense_{k}"]
        kern = d["kernel"] if isinstance(d["kernel"], torch.Tensor) else torch.from_numpy(np.array(d["kernel"]))     # (copy: msgpack buffers are read-only)
        bias = d["bias"] if isinstance(d["bias"], torch.Tensor) else torch.from_numpy(np.array(d["bias"]))
        if tuple(kern.shape) != (i, o) or tuple(bias.shape) != (o,):
            raise ValueError(f"Dense_{k}: expected kernel {(i, o)} / bias {(o,)}, got {tuple(kern.shape)} / {tuple(bias.shape)}")
        parts += [kern.reshape(-1).float(), bias.reshape(-1).float()]
    flat = torch.cat(parts)
    return flat.to(device) if device is not None else flat


def init_mlp_flat(gen: torch.Generator, shapes, out_std: Optional[float] = None) -> torch.Tensor:
    """glorot/xavier-uniform kernels, zero biases (rnerf/model_utils.py:62-63,124); optional N(0, out_std) output layer."""
    parts = []
    for k, (i, o) in enumerate(shapes):
        if out_std is not None and k == len(shapes) - 1:
            kern = torch.randn((i, o), generator=gen) * out_std
        else:
            lim = math.sqrt(6.0 / (i + o))
            kern = (torch.rand((i, o), generator=gen) * 2 - 1) * lim
        parts += [kern.reshape(-1), torch.zeros(o)]
    return torch.cat(parts).float()


class NerfModel:
    """Mirror of rnerf/models.py:NerfModel (attributes :42-90, setup :91-137)."""

    def __init__(self, *, ndim, nmin, nmax, grid, near=2.0, far=6.0, num_coarse_samples=64, num_fine_samples=128,
                 num_path_samples=8, min_deg_point=0, max_deg_point=10, deg_view=4, use_viewdirs=True, white_bkgd=False,
                 stage="radiance", rgb_padding=0.001, sigma_bias=-1.0, noise_std=None, sh_deg=-1, sh_direnc_deg=-1,
                 use_mask_bbox=False, bd_cut_dist=None, cfg_name=None, use_random_choice=True, use_online_sparsity=False,
                 use_fine_sparsity=False, net_depth=8, net_width=256, net_depth_condition=1, net_width_condition=128,
                 skip_layer=4, num_rgb_channels=3, num_sigma_channels=1, legacy_posenc_order=False, lindisp=False,
                 precision="f16x3", eval_precision=None, table_layout="reference", device=None, **unused):
        if not (stage.startswith("radiance") or stage.startswith("all") or stage.startswith("ior")):
            raise NotImplementedError(f"stage={stage!r}: expected radiance*, ior* or all* (rnerf/eikonal_utils.py:34-39, train.py:286-310)")
        if (net_depth, net_width, net_depth_condition, net_width_condition, skip_layer) != (8, 256, 1, 128, 4):
            raise NotImplementedError("the HIP NerfMLP kernel is specialised for the reference's 8x256 / skip 4 / 1x128 network")
        if (min_deg_point, max_deg_point, deg_view) != (0, 10, 4) or legacy_posenc_order or not use_viewdirs:
            raise NotImplementedError("the HIP kernels implement pos_enc degrees (0,10)/(0,4), non-legacy order, use_viewdirs=True")
        if sh_deg >= 0 or sh_direnc_deg > 0:
            raise NotImplementedError("sh_deg / sh_direnc_deg are disabled in every shipped config and not built")
        self.noise_std = None if noise_std is None else float(noise_std)
        if use_mask_bbox and bd_cut_dist is not None:
            raise ValueError("'use_mask_bbox' is true (rnerf/models.py:480: bd_cut_dist and use_mask_bbox exclude each other)")
        # use_mask_bbox (rnerf/models.py:261-271,398-408): density only at samples inside the grid's box [nmin, nmax], in both levels
        self.use_mask_bbox = bool(use_mask_bbox)
        # lindisp: a field of the reference's NerfModel (rnerf/models.py:74) that its __call__ never reads — the samples come from the eikonal
        # march, not from sample_along_rays — so it is accepted and, like there, has no effect
        self.lindisp = bool(lindisp)
        if num_coarse_samples < 3:
            raise ValueError("num_coarse_samples must be >= 3")
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.ndim = [int(v) for v in ndim]; self.nmin = [float(v) for v in nmin]; self.nmax = [float(v) for v in nmax]
        self.near, self.far = float(near), float(far)
        self.num_coarse_samples, self.num_fine_samples = int(num_coarse_samples), int(num_fine_samples)
        self.num_path_samples = int(num_path_samples)
        self.white_bkgd, self.stage = bool(white_bkgd), stage
        self.rgb_padding, self.sigma_bias = float(rgb_padding), float(sigma_bias)
        self.bd_cut_dist, self.cfg_name = bd_cut_dist, cfg_name
        self.use_random_choice = bool(use_random_choice)
        self.use_online_sparsity, self.use_fine_sparsity = bool(use_online_sparsity), bool(use_fine_sparsity)
        self.precision = PRECISIONS[precision]
        # eval_precision: the arithmetic of the pure render pass (apply() without taps / ctx -> ONE rnerf_forward call: eval.py, render_image).
        # None = `precision` (construct_nerf's default since round 6).  "f16f8": the f16 main term + fp8 cross terms, ~6-8 % faster, |dRGB| ~2e-6 of
        # the oracle on glorot weights but 2e-4 on trained-like ones (opt-in, see construct_nerf); a weight outside its range makes the launch fall
        # back to f16x3 on the device, an activation beyond e4m3's 448 sends the row to the range-safe second pass.
        # Training (train_step) and every tapped / staged path always run `precision`.
        if eval_precision is not None and eval_precision not in PRECISIONS:
            raise ValueError(f"eval_precision must be one of {sorted(PRECISIONS)}")
        self.eval_precision = PRECISIONS[eval_precision] if eval_precision is not None else self.precision
        self.coarse_step_size = (self.far - self.near) / self.num_coarse_samples         # rnerf/models.py:133-134
        self.fine_step_size = (self.far - self.near) / (self.num_coarse_samples + self.num_fine_samples)
        self.num_samples = self.num_coarse_samples * self.num_path_samples               # rnerf/models.py:121
        self.step_size = (self.far - self.near) / (self.num_samples - 1)                 # :122
        # table_layout: memory order of the (n, grad n) table (include/rnerf.h: rnerf_table_layout) — "reference" = the reference's flat index,
        # "bricks" = 2x2x2 bricks of one cache line (fewer new lines per march step on tables beyond the caches).  Same values, same indices.
        self.spec = Grid.make(self.ndim, self.nmin, self.nmax, table_layout)
        if device is None:
            device = grid.device if isinstance(grid, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        g = grid if isinstance(grid, torch.Tensor) else torch.as_tensor(np.asarray(grid, np.float32))
        g = g.to(self.device, torch.float32).reshape(self.ndim)
        # VoxMLP.setup: data = concat([grid, grad]) (rnerf/ior_utils.py:161) — built once on the device
        self.table = ops.grid_build_table(g, self.spec)
        self._packed: Dict[str, Tuple[Any, int, torch.Tensor]] = {}
        self._packed_bwd: Dict[str, Tuple[Any, int, torch.Tensor, int]] = {}      # the dgrad streams (train._bwd_packed)
        self._jit_cache: Dict[bytes, Tuple[torch.Tensor, torch.Tensor]] = {}      # _pinned_upload entries: (pinned source, device tensor)
        self._u_lin: Optional[torch.Tensor] = None
        self._side: Optional[torch.cuda.Stream] = None
        self._tail: Optional[torch.cuda.Stream] = None
        self._mlp_wg_limit = 0
        # whole_path: apply() goes through rnerf_forward (one C call per batch); False keeps the stage-by-stage host sequence (tests / taps)
        self.whole_path = True
        self._ws: Dict[Tuple[str, int], torch.Tensor] = {}
        self._key_cache: Dict[bytes, Tuple[torch.Tensor, torch.Tensor]] = {}

    def table_reference(self) -> torch.Tensor:
        """The (n, grad n) table in the reference's order [G^3, 4] whatever layout the kernels use (for the oracle and the tests)."""
        return ops.table_reference_order(self.table, self.spec)

    # ---- parameters -------------------------------------------------------------------------------------------------------
    def init(self, key, **unused) -> Dict[str, Any]:
        """model.init: fresh variables {"params": tree-of-views, "flat": flat fp32 buffers} (rnerf/models.py:611-616)."""
        seed = int(np.asarray(key, np.uint32)[-1]) if key is not None else 0
        gen = torch.Generator().manual_seed(seed)
        flat = {"coarse_mlp": init_mlp_flat(gen, NERF_MLP_SHAPES), "bkgd_mlp": init_mlp_flat(gen, BKGD_MLP_SHAPES)}
        if self.num_fine_samples > 0:
            flat["fine_mlp"] = init_mlp_flat(gen, NERF_MLP_SHAPES)
        flat["so3_mlp"] = init_mlp_flat(gen, SO3_MLP_SHAPES, out_std=1e-5)            # rnerf/ior_utils.py:148-152
        return make_variables({k: v.to(self.device) for k, v in flat.items()})

    def _flat(self, variables, name: str, shapes) -> torch.Tensor:
        f = variables.get("flat", {}).get(name)
        if f is None:
            tree = (variables["params"]["path_sampler"]["scan"]["idx_model"]["so3_mlp"] if name == "so3_mlp" else variables["params"][name])
            f = tree_to_flat(tree, shapes, self.device)
            variables.setdefault("flat", {})[name] = f
        return f

    def _packed_weights(self, variables, name: str, precision: Optional[int] = None) -> torch.Tensor:
        flat = self._flat(variables, name, NERF_MLP_SHAPES)
        prec = self.precision if precision is None else int(precision)
        slot = name if prec == self.precision else (name, prec)          # one cached operand stream per (network, arithmetic)
        ent = self._packed.get(slot)
        # keyed on the tensor OBJECT (weakly) + its version: a data_ptr key would go stale when a freed buffer's address is reused
        if ent is None or ent[0]() is not flat or ent[1] != flat._version:
            buf = ops.nerfmlp_pack(flat.detach(), prec, ent[2] if ent is not None else None)
            self._packed[slot] = (weakref.ref(flat), flat._version, buf)
        return self._packed[slot][2]

    # ---- randomness -------------------------------------------------------------------------------------------------------
    def make_jitter(self, key) -> np.ndarray:
        """jitter = arange(0, N, P) (+ randint(key, [N_c], 0, P)) — rnerf/models.py:240-242 (also when randomized=False)."""
        j = np.arange(0, self.num_samples, self.num_path_samples, dtype=np.int32)
        if self.use_random_choice:
            j = j + prng.randint(key, (self.num_coarse_samples,), 0, self.num_path_samples)
        return j.astype(np.int32)

    def _jitter_dev(self, jitter) -> torch.Tensor:
        j = np.ascontiguousarray(np.asarray(jitter, np.int32))
        if j.shape != (self.num_coarse_samples,) or j.min() < 0 or j.max() >= self.num_samples:
            raise ValueError("jitter must be int[N_c] with values in [0, N_c*P)")
        if np.any(np.diff(j) <= 0):
            raise ValueError("jitter must be strictly increasing")
        return self._pinned_upload(self._jit_cache, j)

    def _pinned_upload(self, cache: Dict[bytes, Tuple[torch.Tensor, torch.Tensor]], host: np.ndarray) -> torch.Tensor:
        """A small host array as a device tensor, cached by value.  Pinned staging + asynchronous copy: a pageable H2D copy would block the host until
        the stream drains, i.e. once per training step (the jitter is redrawn every step); the entry keeps the pinned buffer alive until evicted."""
        b = host.tobytes()
        ent = cache.get(b)
        if ent is None:
            if len(cache) > 64:
                cache.clear()
            pin = torch.from_numpy(host).pin_memory()
            ent = cache[b] = (pin, pin.to(self.device, non_blocking=True))
        return ent[1]

    def make_u(self, key, batch: int, randomized: bool):
        """The uniform draws of sorted_piecewise_constant_pdf (rnerf/model_utils.py:343-356), sample-major."""
        F = self.num_fine_samples
        if not randomized:
            if self._u_lin is None:
                u = np.linspace(0.0, 1.0 - float(np.finfo(np.float32).eps), F).astype(np.float32)
                self._u_lin = torch.from_numpy(u).to(self.device)
            return self._u_lin
        return ops.stratified_u(np.asarray(key, np.uint32), batch, F, self.device)

    def make_u_host(self, key, batch: int) -> np.ndarray:
        """numpy form of the randomized branch (what rnerf_stratified_u computes on the device); [F, B]."""
        F = self.num_fine_samples
        eps = float(np.finfo(np.float32).eps)
        s = 1.0 / F
        u = (np.arange(F, dtype=np.float32) * np.float32(s))[None, :] + prng.uniform(key, (batch, F), maxval=s - eps)
        return np.ascontiguousarray(np.minimum(u, np.float32(1.0 - eps)).astype(np.float32).T)

    def _mask_bbox(self):
        """use_mask_bbox's box: the grid's own (rnerf/models.py:262-264, "small mask bbox")."""
        return list(self.nmin) + list(self.nmax)

    def _bd_cut_bbox(self):
        """The scene-name-specific box of rnerf/models.py:485-497."""
        name = self.cfg_name or ""
        nmin, nmax = list(self.nmin), list(self.nmax)
        if "pen" in name:
            nmax[1] -= 0.6
        elif "ball" in name:
            nmin, nmax = [-1, 0.03597, -1], [1, 2.03597, 1]
        elif "glass" in name:
            nmax[1] -= 0.7
        else:
            raise NotImplementedError("bd_cut_dist is defined for the pen / ball / glass configs only (rnerf/models.py:485-497)")
        return nmin + nmax

    # ---- cross-batch pipelining ---------------------------------------------------------------------------------------------
    def prefetch_path(self, rays: Rays, sync_inputs: bool = True, reserve_cus: int = 32) -> "PathHandle":
        """March `rays` on a side stream so that it overlaps the MLP phase of the batch currently in flight.

        The march is a latency-bound dependent gather chain (256 waves at B = 4096) and needs no matrix core; the MLP
        kernel is MFMA-bound and owns whole CUs.  `reserve_cus` CUs are kept free of MLP workgroups so both can run at
        once.  Pass the handle to `apply(..., path=handle)` (same rays).  sync_inputs=False skips the wait on the current
        stream when the ray tensors are known to be complete already (e.g. slices of a resident image)."""
        if not self.stage.startswith("radiance"):
            raise NotImplementedError("prefetch_path: the all* march depends on the so3_mlp parameters; call apply() without a handle")
        if self._side is None:
            self._side = shared_stream(self.device, "march")
        # per-model cap of the MLP kernels' persistent grid, passed with every rnerf_nerfmlp_forward call (0 = every CU)
        self._mlp_wg_limit = max(_lib.load().rnerf_device_cus() - int(reserve_cus), 1) if reserve_cus > 0 else 0
        cur = torch.cuda.current_stream()
        if sync_inputs:
            self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            # the caller may drop its ray tensors before the side stream has marched them: keep the allocator from reusing that memory
            rays.origins.record_stream(self._side); rays.viewdirs.record_stream(self._side)
            pd, dr, ior, _ = ops.march(self.table, self.spec, rays.origins, rays.viewdirs, self.near, self.far,
                                       self.num_samples, want_ior=self.use_online_sparsity)
            ev = torch.cuda.Event()
            ev.record(self._side)
        return PathHandle(pd, dr, ior, ev, rays.origins.shape[0])

    def prefetch_slot(self, rays: Rays, next_keys=None):
        """A PathHandle whose march rnerf_train_forward_backward issues itself (rnerf_prefetch): buffers + descriptor; the caller records
        handle.event on the side stream after the call.  next_keys = (key_0, key_1) of the step that will consume the path (flat models):
        the march draws that step's jitter into a buffer of the handle and records only its nodes (a sparse handle)."""
        if not self.stage.startswith("radiance"):
            raise NotImplementedError("prefetch: the all* march depends on the so3_mlp parameters")
        if self._side is None:
            self._side = shared_stream(self.device, "march")
        o, v = ops._chk(rays.origins, "origins"), ops._chk(rays.viewdirs, "viewdirs")
        B = o.shape[0]
        pd = torch.empty((self.num_samples, B, 4), dtype=torch.float32, device=self.device)
        dr = torch.empty_like(pd)
        for t in (o, v, pd, dr):
            t.record_stream(self._side)
        h = PathHandle(pd, dr, None, torch.cuda.Event(), B)
        h.keep = (o, v)
        nxt = _lib.Prefetch(o.data_ptr(), v.data_ptr(), pd.data_ptr(), dr.data_ptr(), self._side.cuda_stream)
        if next_keys is not None:
            if self.num_fine_samples > 0:
                raise ValueError("prefetch_slot: a hierarchical model resamples arbitrary nodes and needs every record (next_keys=None)")
            keys = self._keys_dev(*next_keys)
            jit = torch.empty(self.num_coarse_samples, dtype=torch.int32, device=self.device)
            keys.record_stream(self._side); jit.record_stream(self._side)
            h.sparse, h.jitter, h.key = True, jit, np.array(next_keys[0], np.uint32).reshape(2).copy()
            h.keep = (o, v, keys)
            h._march_args = (self.table, self.spec, self.near, self.far, self.num_samples)      # what complete() marches the other nodes with
            nxt.next_keys4, nxt.sample_nodes = keys.data_ptr(), jit.data_ptr()
        return h, nxt

    def tail_stream(self) -> torch.cuda.Stream:
        """The stream rnerf_train_forward_backward uses for work that is independent of the NerfMLP backward (rnerf_train_cfg.aux_stream)."""
        if self._tail is None:
            self._tail = shared_stream(self.device, "tail")
        return self._tail

    def comm_stream(self) -> torch.cuda.Stream:
        """The stream the train step's NerfMLP-gradient all-reduce is issued from (rnerf_train_cfg.grads_stream: ordered behind the last wgrad).
        It IS the tail stream: that one is idle from the step's last join to the next step's first fork — exactly where the collective is
        issued (the process group runs it on a stream of its own and only takes its ordering from here) —, and one stream fewer is one
        hardware queue more for the others (shared_stream)."""
        return self.tail_stream()

    def release_reserved_cus(self) -> None:
        """Give the CUs reserved by prefetch_path(reserve_cus > 0) back to the MLP kernels."""
        self._mlp_wg_limit = 0

    # ---- the whole path in one call (csrc/pipeline.hip) ------------------------------------------------------------------------
    def c_model(self, variables=None, precision: Optional[int] = None) -> "_lib.Model":
        """The rnerf_model descriptor of this model (+ the packed weights of `variables`, when given); precision: override (eval_precision)."""
        prec = self.precision if precision is None else int(precision)
        m = _lib.Model()
        m.table = self.table.data_ptr()
        m.grid = self.spec
        m.near, m.far = self.near, self.far
        m.num_coarse, m.num_fine, m.num_path = self.num_coarse_samples, self.num_fine_samples, self.num_path_samples
        m.precision, m.white_bkgd = int(prec), int(self.white_bkgd)
        m.rgb_padding, m.sigma_bias = self.rgb_padding, self.sigma_bias
        m.bd_cut = int(self.bd_cut_dist is not None and self.num_fine_samples > 0)
        if m.bd_cut:
            for i, v in enumerate(self._bd_cut_bbox()):
                m.bd_cut_bbox[i] = float(v)
        elif self.use_mask_bbox:          # rnerf_model.bd_cut = 2: the per-sample box mask of both levels, the box in bd_cut_bbox
            m.bd_cut = 2
            for i, v in enumerate(self._mask_bbox()):
                m.bd_cut_bbox[i] = float(v)
        if variables is not None:
            m.packed_coarse = self._packed_weights(variables, "coarse_mlp", prec).data_ptr()
            if self.num_fine_samples > 0:
                m.packed_fine = self._packed_weights(variables, "fine_mlp", prec).data_ptr()
            m.bkgd_params = self._flat(variables, "bkgd_mlp", BKGD_MLP_SHAPES).detach().data_ptr()
        return m

    def _workspace(self, kind: str, nbytes: int) -> torch.Tensor:
        """One cached scratch buffer per kind ("fwd" / "train"), grown on demand (calls on one stream are ordered, so it is reused)."""
        t = self._ws.get(kind)
        if t is None or t.numel() < nbytes:
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._ws[kind] = t
        return t

    def _keys_dev(self, *keys) -> torch.Tensor:
        """jax.random keys as a device uint32 vector (pinned staging, asynchronous copy, cached by value like the jitter)."""
        k = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint32).reshape(2) for x in keys]))
        return self._pinned_upload(self._key_cache, k.view(np.int32))

    def _forward_whole(self, variables, rng_0, rng_1, rays: Rays, randomized: bool, jitter, u_fine, path):
        """NerfModel.__call__ through rnerf_forward: the keys go to the device, every stage is sequenced there."""
        lib = _lib.load()
        o, v = ops._chk(rays.origins, "origins"), ops._chk(rays.viewdirs, "viewdirs")
        B, Nc, Nf = o.shape[0], self.num_coarse_samples, self.num_fine_samples
        st = _lib.current_stream()
        m = self.c_model(variables, self.eval_precision)
        keys = None
        if jitter is None:
            keys = self._keys_dev(rng_0, rng_1)
            jit = torch.empty(Nc, dtype=torch.int32, device=self.device)
            key_u = torch.empty(2, dtype=torch.int32, device=self.device)
            _lib.check(lib.rnerf_rng_forward(keys.data_ptr(), Nc, self.num_path_samples, int(self.use_random_choice), jit.data_ptr(), key_u.data_ptr(), st),
                       "rnerf_rng_forward")
        else:
            jit = self._jitter_dev(jitter)
        u, per_ray = None, 0
        if Nf > 0:
            if u_fine is not None:
                u = ops._chk(u_fine, "u_fine"); per_ray = 1 if u.dim() == 2 else 0
            elif not randomized:
                u = self.make_u(None, B, False)
            else:
                if jitter is not None:          # the key chain was not run on the device: derive the stratified key on the host
                    key, _ = prng.split(np.asarray(rng_1, np.uint32))
                    u = self.make_u(key, B, True)
                else:
                    u = torch.empty((Nf, B), dtype=torch.float32, device=self.device)
                    _lib.check(lib.rnerf_stratified_u_dev(key_u.data_ptr(), B, Nf, u.data_ptr(), st), "rnerf_stratified_u_dev")
                per_ray = 1
        pd, dr = path.adopt(B) if path is not None else (None, None)
        ws = self._workspace("fwd", lib.rnerf_forward_workspace_bytes(C.byref(m), B))
        out_c = torch.empty(_lib.LEVEL_FLOATS * B, dtype=torch.float32, device=self.device)
        out_f = torch.empty(_lib.LEVEL_FLOATS * B, dtype=torch.float32, device=self.device) if Nf > 0 else None
        _lib.check(lib.rnerf_forward(C.byref(m), o.data_ptr(), v.data_ptr(), B, jit.data_ptr(), _lib.ptr(u), per_ray, _lib.ptr(pd), _lib.ptr(dr),
                                     out_c.data_ptr(), _lib.ptr(out_f), ws.data_ptr(), int(self._mlp_wg_limit), st), "rnerf_forward")
        return [level_views(t, B) for t in (out_c, out_f) if t is not None]

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def apply(self, variables, *args, method=None, **kwargs):
        """flax-style entry: model.apply(variables, rng_0, rng_1, rays, randomized[, annealed_alpha]) or
        model.apply(variables, viewdirs, method=model.forward_envmap) (rnerf/train.py:81,129)."""
        if method is not None:
            return method(variables, *args, **kwargs)
        return self.forward(variables, *args, **kwargs)

    def forward(self, variables, rng_0, rng_1, rays: Rays, randomized: bool, annealed_alpha: float = 1.0, *,
                jitter=None, u_fine: Optional[torch.Tensor] = None, taps: Optional[dict] = None,
                path: Optional["PathHandle"] = None, ctx: Optional[dict] = None,
                noise_c: Optional[torch.Tensor] = None, noise_f: Optional[torch.Tensor] = None):
        """NerfModel.__call__ (rnerf/models.py:220-535).

        noise_c [B, Nc] / noise_f [B, Nc + Nf]: the standard-normal draws of the raw-sigma regulariser given explicitly (tests); drawn from
        the key chain like the reference otherwise.  Used only when noise_std is set and `randomized`.

        ctx: a dict to fill with what the backward pass needs (samplenerfro_amd.train); the MLPs then run their training
        forward, which also stores the MFMA operands of every layer."""
        origins, viewdirs = rays.origins, rays.viewdirs                                   # rnerf/models.py:235-236
        if origins.dim() != 2 or origins.shape[-1] != 3:
            raise ValueError("rays.origins must be [B, 3]")
        B = origins.shape[0]
        noisy = self.noise_std is not None and randomized                                 # add_gaussian_noise (rnerf/model_utils.py:438-453)
        if ctx is None and taps is None and self.whole_path and self.stage.startswith("radiance") and not self.use_online_sparsity and not noisy:
            # the product path: ONE call into librnerf.so (rnerf_forward) sequences every stage on the device; the stage-by-stage
            # code below is the same sequence with taps, kept for the parity tests and for the variants rnerf_forward does not cover
            return self._forward_whole(variables, rng_0, rng_1, rays, randomized, jitter, u_fine, path), 0.0
        Nc, Nf, N = self.num_coarse_samples, self.num_fine_samples, self.num_samples
        key, rng_0 = prng.split(np.asarray(rng_0, np.uint32))
        # loss_sp (rnerf/models.py:351-357,526-530): always in a pure forward; in a training forward only when the caller asks for its VALUE
        # (ctx["loss_sp"], set by train_step with taps) — train.py:156 multiplies the term by annealing_rate = 0.0, so neither the loss nor any
        # gradient depends on it and the product step does not pay for the IoR record it would need
        sparsity = self.use_online_sparsity and (ctx is None or (bool(ctx.get("loss_sp")) and not self.stage.startswith("all")))
        want_ior = sparsity or (taps is not None and not (ctx is not None and self.stage.startswith("all")))
        if path is not None:
            (path_pd, path_dr), path_ior = path.adopt(B), path.ior
            if want_ior and path_ior is None:
                raise ValueError("path handle lacks the IoR record (prefetch it from a model with the same options)")
        elif self.stage.startswith("all") and ctx is not None:                            # training: the march also records what its adjoint needs
            rec = ops.march_all_train(self.table, self.spec, self._flat(variables, "so3_mlp", SO3_MLP_SHAPES).detach(), origins, viewdirs,
                                      self.near, self.far, N, annealed_alpha, lazy=True)      # pairs finalised by train._all_stage_backward
            ctx["march_rec"] = rec
            path_pd, path_dr, path_ior = rec["path_pd"], rec["path_dr"], None
            if want_ior:
                raise NotImplementedError("taps / online sparsity are not recorded by the training march of stage all*")
        elif self.stage.startswith("all"):                                                # so3_mlp bends the gradient (eikonal_utils.py:34-39)
            path_pd, path_dr, path_ior = ops.march_all(self.table, self.spec, self._flat(variables, "so3_mlp", SO3_MLP_SHAPES).detach(),
                                                       origins, viewdirs, self.near, self.far, N, annealed_alpha, want_ior=want_ior)
        else:
            path_pd, path_dr, path_ior, _ = ops.march(self.table, self.spec, origins, viewdirs, self.near, self.far, N,
                                                      want_ior=want_ior)
        if jitter is None:
            jitter = self.make_jitter(key)
        jit = self._jitter_dev(jitter)
        last = int(np.asarray(jitter)[-1])
        # bkgd from the LAST coarse sample's direction (rnerf/models.py:303)
        bkgd_flat = self._flat(variables, "bkgd_mlp", BKGD_MLP_SHAPES).detach()
        if ctx is None:
            bkgd = ops.bkgd_forward(bkgd_flat, path_dr[last], self.rgb_padding)
            raw_c = ops.nerfmlp_forward(self._packed_weights(variables, "coarse_mlp"), self.precision, path_pd, path_dr, jit, Nc, B,
                                        max_workgroups=self._mlp_wg_limit)
        else:
            env = ctx.get("env_dirs")
            if env is None:
                bkgd, ctx["save_bkgd"] = ops.bkgd_forward_train(bkgd_flat, path_dr[last], self.rgb_padding)
            else:
                # the env-map patch of train.py:127-130 rides in the same launch: rows [0, B) = the rays' last coarse direction,
                # rows [B, B + M) = the patch directions; one training forward, later one backward, for both
                both = torch.cat([path_dr[last][:, :3], env], 0)
                out, ctx["save_bkgd"] = ops.bkgd_forward_train(bkgd_flat, both, self.rgb_padding)
                bkgd, ctx["rgb_env"] = out[:B], out[B:]
            raw_c, ctx["save_c"] = ops.nerfmlp_forward_train(self._packed_weights(variables, "coarse_mlp"), self.precision, path_pd,
                                                            path_dr, jit, Nc, B, ctx.get("backward", _lib.BWD_F16X2),
                                                            max_workgroups=self._mlp_wg_limit)
        if noisy:                                                                         # rnerf/models.py:310-317: the key chain advances only here
            key, rng_0 = prng.split(rng_0)
            raw_c = self._add_sigma_noise(raw_c, key, noise_c)
        if ctx is not None:
            ctx.update(path_pd=path_pd, path_dr=path_dr, jit=jit, raw_c=raw_c, bkgd=bkgd, B=B)
        mb = self._mask_bbox() if self.use_mask_bbox else None
        if ctx is not None and mb is not None:
            ctx["mask_bbox"] = mb
        rgb, dist, acc, trans, trans_bkgd, weights, alpha = ops.composite(
            raw_c, path_pd, path_dr, jit, Nc, B, bkgd, self.white_bkgd, self.rgb_padding, self.sigma_bias,
            want_weights=True, want_alpha=sparsity, mask_mode=3 if mb is not None else 0, bbox=mb)
        loss_sp = 0.0
        if sparsity:                                                      # rnerf/models.py:351-357
            g = path_ior[jit.long()][..., 1:4]
            mask = (torch.sqrt((g * g).sum(-1)) > 1e-6).float()
            loss_sp = (mask * torch.log(torch.clamp(alpha, min=1e-6))).sum() / (mask.sum() + 1)
        ret = [(rgb, dist, acc, trans, trans_bkgd)]
        if taps is not None:
            taps.update(path_pd=path_pd, path_dr=path_dr, path_ior=path_ior, jitter=np.asarray(jitter), raw_c=raw_c,
                        weights_c=weights, bkgd=bkgd)
        if Nf > 0:
            key, rng_1 = prng.split(np.asarray(rng_1, np.uint32))
            u = u_fine if u_fine is not None else self.make_u(key, B, randomized)
            fine_sp = sparsity and self.use_fine_sparsity
            rows_pd, rows_dr, idx = ops.resample(path_pd, path_dr, jit, weights, u, Nf, want_idx=(taps is not None) or fine_sp)
            S = Nc + Nf
            if ctx is None:
                raw_f = ops.nerfmlp_forward(self._packed_weights(variables, "fine_mlp"), self.precision, rows_pd, rows_dr, None, S, B,
                                            max_workgroups=self._mlp_wg_limit)
            else:
                raw_f, ctx["save_f"] = ops.nerfmlp_forward_train(self._packed_weights(variables, "fine_mlp"), self.precision, rows_pd,
                                                                rows_dr, None, S, B, ctx.get("backward", _lib.BWD_F16X2),
                                                                max_workgroups=self._mlp_wg_limit)
            if noisy:                                                                     # rnerf/models.py:445-452
                key, rng_1 = prng.split(rng_1)
                raw_f = self._add_sigma_noise(raw_f, key, noise_f)
            if ctx is not None:
                ctx.update(rows_pd=rows_pd, rows_dr=rows_dr, raw_f=raw_f)
            rgb, dist, acc, trans, trans_bkgd, w_f, alpha_f = ops.composite(
                raw_f, rows_pd, rows_dr, None, S, B, bkgd, self.white_bkgd, self.rgb_padding, self.sigma_bias,
                want_weights=taps is not None, want_alpha=fine_sp, mask_mode=3 if mb is not None else 0, bbox=mb)
            if fine_sp:                                                                   # rnerf/models.py:526-530
                g = path_ior[idx.long(), torch.arange(B, device=self.device)[None, :]][..., 1:4]
                mask = (torch.sqrt((g * g).sum(-1)) > 1e-6).float()
                loss_sp = loss_sp + (mask * torch.log(torch.clamp(alpha_f, min=1e-6))).sum() / (mask.sum() + 1)
            if self.bd_cut_dist is not None:                                              # rnerf/models.py:479-524
                bbox = self._bd_cut_bbox()
                # trans with the density kept only up to the last sample inside the box (rgb_bkgd=None)
                _, _, _, trans, _, _, _ = ops.composite(raw_f, rows_pd, rows_dr, None, S, B, None, self.white_bkgd, self.rgb_padding,
                                                        self.sigma_bias, want_weights=False, mask_mode=1, bbox=bbox)
                # colour of everything BEHIND the box over the background, then attenuated by that trans
                behind, _, _, _, _, _, _ = ops.composite(raw_f, rows_pd, rows_dr, None, S, B, bkgd, self.white_bkgd, self.rgb_padding,
                                                         self.sigma_bias, want_weights=False, mask_mode=2, bbox=bbox)
                trans_bkgd = trans * behind
                if ctx is not None:
                    ctx["bd_cut_bbox"] = bbox
            ret.append((rgb, dist, acc, trans, trans_bkgd))
            if taps is not None:
                taps.update(rows_pd=rows_pd, rows_dr=rows_dr, idx_f=idx, raw_f=raw_f, weights_f=w_f, u=u)
        return ret, loss_sp

    def _add_sigma_noise(self, raw: torch.Tensor, key, given: Optional[torch.Tensor]) -> torch.Tensor:
        """raw [S, B, 4]: raw sigma += noise_std * N(0, 1), drawn in the reference's [B, S, 1] order (rnerf/model_utils.py:438-453).  In place:
        the regulariser is additive, so the MLP backward is untouched and the composite's backward differentiates at the noisy raw."""
        S, B = raw.shape[0], raw.shape[1]
        z = prng.normal(key, (B, S)) if given is None else given
        z = torch.as_tensor(z, dtype=torch.float32).to(raw.device, non_blocking=True).reshape(B, S)
        raw[..., 3] += self.noise_std * z.t()
        return raw

    __call__ = forward

    def forward_envmap(self, variables, viewdirs: torch.Tensor, ctx: Optional[dict] = None) -> torch.Tensor:
        """rnerf/models.py:181-191: bkgd colour for arbitrary view directions [M,3] -> [M,3]."""
        if ctx is not None:
            out, ctx["save_env"] = ops.bkgd_forward_train(self._flat(variables, "bkgd_mlp", BKGD_MLP_SHAPES).detach(), viewdirs,
                                                          self.rgb_padding)
            return out
        return ops.bkgd_forward(self._flat(variables, "bkgd_mlp", BKGD_MLP_SHAPES).detach(), viewdirs, self.rgb_padding)


    # ---- auxiliary entry points (rnerf/models.py:142-218), forward only -------------------------------------------------------
    def _point_query(self, variables, mlp: str, pts: torch.Tensor, viewdirs: torch.Tensor):
        """PE + NerfMLP on free-standing points: pts [..., 3], viewdirs [..., 3] (broadcast against pts) -> raw [n, 4]."""
        p = pts.reshape(-1, 3)
        v = viewdirs.expand(*pts.shape[:-1], 3).reshape(-1, 3) if viewdirs.shape != pts.shape else viewdirs.reshape(-1, 3)
        n = p.shape[0]
        z = torch.zeros((n, 1), dtype=torch.float32, device=p.device)
        pd = torch.cat([p.float(), z], -1).reshape(1, n, 4).contiguous()
        dr = torch.cat([v.float(), z], -1).reshape(1, n, 4).contiguous()
        return ops.nerfmlp_forward(self._packed_weights(variables, mlp), self.precision, pd, dr, None, 1, n).reshape(n, 4)

    def sample_points(self, variables, pts: torch.Tensor, viewdirs: torch.Tensor):
        """rnerf/models.py:193-218 (used by extract_mesh.py:243): colour and per-step alpha of the fine (or coarse) field at points."""
        fine = self.num_fine_samples > 0
        raw = self._point_query(variables, "fine_mlp" if fine else "coarse_mlp", pts, viewdirs)
        step = self.fine_step_size if fine else self.coarse_step_size
        rgb = torch.sigmoid(raw[:, :3]) * (1 + 2 * self.rgb_padding) - self.rgb_padding
        sigma = torch.nn.functional.softplus(raw[:, 3:4] + self.sigma_bias)
        alpha = 1 - torch.exp(-step * sigma)
        return rgb.reshape(*pts.shape[:-1], 3), alpha.reshape(*pts.shape[:-1], 1)

    def wrapper_compute_normal_loss_and_smooth(self, variables, ray_pos: torch.Tensor, idx_grad: torch.Tensor, annealed_alpha: float = 1.0,
                                               noise: Optional[torch.Tensor] = None):
        """E4: PathSampler.compute_normal_loss_and_smooth (rnerf/eikonal_utils.py:84-98; rnerf/models.py:139-140), forward only:
        (0.0, mean sum_c |so3-rotated(idx_grad) at x - at x + noise * ndelta| / |idx_grad|).  noise [..., 3]: the standard-normal draw
        scaled by normal_radius_scale = 0.1 (the reference takes it from numpy's global RNG; default: torch.randn * 0.1)."""
        so3 = self._flat(variables, "so3_mlp", SO3_MLP_SHAPES).detach()
        x = ray_pos.reshape(-1, 3).float().contiguous(); g = idx_grad.reshape(-1, 3).float().contiguous()
        if noise is None:
            noise = 0.1 * torch.randn_like(x)
        ndelta = torch.tensor([(self.nmax[i] - self.nmin[i]) / (self.ndim[i] - 1.0) for i in range(3)], dtype=torch.float32, device=x.device)
        _, pred = ops.so3_query(self.table, self.spec, so3, x, annealed_alpha, condition=g)
        _, pred_r = ops.so3_query(self.table, self.spec, so3, (x + noise.reshape(-1, 3).float() * ndelta).contiguous(), annealed_alpha, condition=g)
        factor = torch.sqrt(torch.clamp((g * g).sum(-1, keepdim=True), min=1e-6))
        return 0.0, ((pred - pred_r).abs() / factor).sum(-1, keepdim=True).mean()

    def compute_sparsity_loss(self, variables, ray_pos: torch.Tensor, coarse_alpha_target, fine_alpha_target):
        """rnerf/models.py:142-179 (train.py:116, the offline sparsity term): view direction zero, alpha vs a running target."""
        zero_dir = torch.zeros_like(ray_pos)

        def alpha_of(mlp, step):
            raw = self._point_query(variables, mlp, ray_pos, zero_dir)
            return 1 - torch.exp(-step * torch.nn.functional.softplus(raw[:, 3] + self.sigma_bias))

        alpha = alpha_of("coarse_mlp", self.coarse_step_size)
        loss_sp = (alpha - coarse_alpha_target).abs().mean()
        next_c, next_f = alpha.mean(), 0.0
        if self.num_fine_samples > 0 and self.use_fine_sparsity:
            alpha = alpha_of("fine_mlp", self.fine_step_size)
            loss_sp = loss_sp + (alpha - fine_alpha_target).abs().mean()
            next_f = alpha.mean()
        return loss_sp, next_c, next_f


def level_views(out: torch.Tensor, B: int):
    """The 5-tuple of one level (rnerf/models.py:359-361) as views of a RNERF_LEVEL_FLOATS * B output buffer."""
    return (out[:3 * B].view(B, 3), out[3 * B:4 * B], out[4 * B:5 * B], out[5 * B:6 * B].view(B, 1), out[6 * B:9 * B].view(B, 3))


class PathHandle:
    """A marched path record produced on the side stream (NerfModel.prefetch_path).

    sparse: only the nodes in `jitter` (device int32[N_c], drawn from `key` = the key_0 of the step the path is for) hold records; the
    rest of the buffers is whatever they held.  Such a path may be read through that very jitter only: train_step's flat product path
    does, through raw(), after comparing `key` with the key it derives itself; model.apply refuses it (need_dense()).
    `pd` / `dr` are the WHOLE record [N, B, 4], as they always were: read on a sparse handle they first complete it (complete())."""

    def __init__(self, pd, dr, ior, event, batch, sparse=False, jitter=None, key=None):
        self._pd, self._dr, self.ior, self.event, self.batch = pd, dr, ior, event, batch
        self.sparse, self.jitter, self.key = bool(sparse), jitter, key
        self._march_args = None

    def raw(self):
        """(pd, dr) as the march left them: on a sparse handle only the nodes in `jitter` hold records."""
        return self._pd, self._dr

    @property
    def pd(self):
        self.complete()
        return self._pd

    @property
    def dr(self):
        self.complete()
        return self._dr

    def complete(self) -> None:
        """A sparse handle becomes a dense one: the nodes its march did not record are marched now, on the current stream (a stand-alone
        dense march into scratch, copied to those nodes only — the records of `jitter`'s nodes stay the ones the prefetch wrote, which
        are the same bits).  Not on any step's path: for callers that look at the record itself."""
        if not self.sparse:
            return
        if self._march_args is None:
            raise ValueError("this sparse path handle does not know its rays: it cannot be completed")
        table, spec, near, far, N = self._march_args
        cur = torch.cuda.current_stream()
        cur.wait_event(self.event)
        pd, dr, _, _ = ops.march(table, spec, self.keep[0], self.keep[1], near, far, N)
        rest = torch.ones(N, dtype=torch.bool, device=pd.device)
        rest[self.jitter.long()] = False
        self._pd[rest] = pd[rest]
        self._dr[rest] = dr[rest]
        self._pd.record_stream(cur); self._dr.record_stream(cur)
        self.sparse = False

    def adopt(self, batch: int, raw: bool = False, who: str = "NerfModel.apply"):
        """Hand the record of `batch` rays to the current stream -> (pd, dr): it waits for the march and is recorded as a reader of the buffers
        (ior / jitter too, where present).  raw=True: as the march left them, the only way to read a sparse handle (refused otherwise)."""
        if self.batch != batch:
            raise ValueError("path handle was marched for a different batch size")
        if not raw:
            self.need_dense(who)
        cur = torch.cuda.current_stream()
        cur.wait_event(self.event)
        for t in (self._pd, self._dr, self.ior, self.jitter):
            if t is not None:
                t.record_stream(cur)
        return self._pd, self._dr                  # (a dense handle's pd / dr; a sparse one's would complete it first)

    def need_dense(self, who: str) -> None:
        if self.sparse:
            raise ValueError(f"{who}: this path handle holds the records of its own jitter's nodes only (a flat train step's prefetch); "
                             "march the rays with prefetch_path() or pass path=None")

    def matches(self, key_0) -> bool:
        """A sparse path: was its jitter drawn from this key_0?"""
        return self.key is not None and np.array_equal(np.asarray(self.key, np.uint32).reshape(-1), np.asarray(key_0, np.uint32).reshape(-1))


def make_variables(flat: Dict[str, torch.Tensor]) -> Dict[str, Any]:
    """{"params": flax-shaped tree of views, "flat": the flat buffers the kernels read}."""
    params: Dict[str, Any] = {"coarse_mlp": flat_to_tree(flat["coarse_mlp"], NERF_MLP_SHAPES),
                              "bkgd_mlp": flat_to_tree(flat["bkgd_mlp"], BKGD_MLP_SHAPES)}
    if "fine_mlp" in flat:
        params["fine_mlp"] = flat_to_tree(flat["fine_mlp"], NERF_MLP_SHAPES)
    if "so3_mlp" in flat:
        params["path_sampler"] = {"scan": {"idx_model": {"so3_mlp": flat_to_tree(flat["so3_mlp"], SO3_MLP_SHAPES)}}}
    return {"params": params, "flat": dict(flat)}


def construct_nerf(key, example_batch, args, ndim, nmin, nmax, grid, precision: str = "f16x3", device=None, eval_precision: Optional[str] = None):
    """rnerf/models.py:538-618: build the model and initial variables.  `args` is a flags namespace (utils.default_flags).
    precision: the arithmetic of training and of every tapped path (fp32-grade f16x3); eval_precision: the arithmetic of the pure render pass
    (model.apply as eval.py / render_image call it) — None (the default since round 6) = the same as `precision`.  "f16f8" (f16 main term +
    fp8 cross terms, ~6 % faster per frame) was the default of rounds 4-5 on the strength of glorot-initialised weights (|dRGB| 2e-6); on
    weights shaped like a trained network's — hidden kernels x 1.5, biases N(0, 0.3) — it measures 2e-4, OUTSIDE the 1e-4 contract
    (tests/test_gpu_parity.py::test_render_arithmetics_on_trained_like_weights): opt-in now."""
    if args.rgb_activation != "sigmoid" or args.sigma_activation != "softplus" or args.net_activation != "relu":
        raise NotImplementedError("the HIP kernels implement relu / sigmoid / softplus (the reference defaults, rnerf/utils.py:168-175)")
    if args.sh_deg >= 0 and args.use_viewdirs:
        raise AssertionError("You can only use up to one of: SH or use_viewdirs.")        # rnerf/models.py:571-574
    model = NerfModel(
        min_deg_point=args.min_deg_point, max_deg_point=args.max_deg_point, deg_view=args.deg_view,
        num_coarse_samples=args.num_coarse_samples, num_fine_samples=args.num_fine_samples, use_viewdirs=args.use_viewdirs,
        sh_deg=args.sh_deg, near=args.near, far=args.far, noise_std=args.noise_std, white_bkgd=args.white_bkgd,
        net_depth=args.net_depth, net_width=args.net_width, net_depth_condition=args.net_depth_condition,
        net_width_condition=args.net_width_condition, skip_layer=args.skip_layer, num_rgb_channels=args.num_rgb_channels,
        num_sigma_channels=args.num_sigma_channels, lindisp=args.lindisp, legacy_posenc_order=args.legacy_posenc_order,
        ndim=ndim, nmin=nmin, nmax=nmax, grid=grid, stage=args.stage, num_path_samples=args.num_path_samples,
        use_fine_sparsity=args.use_fine_sparsity, use_online_sparsity=args.use_online_sparsity,
        sh_direnc_deg=args.sh_direnc_deg, cfg_name=args.config, precision=precision, eval_precision=eval_precision, device=device,
        bd_cut_dist=getattr(args, "bd_cut_dist", None),
        use_mask_bbox=getattr(args, "use_mask_bbox", False))      # (both gin-bound attributes of NerfModel in the reference, configs/*.gin)
    key1, _key2, _key3 = prng.split(np.asarray(key, np.uint32), 3)
    return model, model.init(key1)
