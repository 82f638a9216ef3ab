"""The float64 references of tests/helpers/all_backward_ref.py, proven before they judge a kernel (no GPU): chained the way
train._all_stage_backward chains the kernels — so3 Jacobians -> pair Jacobians -> reverse scan -> so3 parameter gradient — they must
reproduce plain autograd of sum(a_pos . ray_pos + a_dir . ray_dir) through the whole march (TR.path_sampler_all) w.r.t. so3_flat."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import all_backward_ref as AR          # noqa: E402
from oracle import ref_np as R, torch_ref as TR          # noqa: E402
from samplenerfro_amd import synthetic as syn          # noqa: E402

F64 = torch.float64


def _scene(ndim, nmin, nmax, B, seed=5):
    a = [np.linspace(nmin[i], nmax[i], ndim[i]) for i in range(3)]
    x, y, z = np.meshgrid(*a, indexing="ij")
    h = min((nmax[i] - nmin[i]) / (ndim[i] - 1) for i in range(3))
    raw = 1.0 + 0.5 * np.clip((0.6 - np.sqrt(x * x + y * y + z * z)) / h + 0.5, 0.0, 1.0)
    grid = R.conv3d_normal(raw.reshape(-1, 1), ndim, 3, 1.0, dtype=np.float64).reshape(ndim)
    table = torch.tensor(R.build_table(grid, ndim, nmin, nmax, dtype=np.float64), dtype=F64)
    rng = np.random.default_rng(seed)
    so3 = syn.init_mlp_flat(rng, TR.SO3_MLP_SHAPES, 0.05)
    so3[-(128 * 3 + 3):-3] = (0.05 * rng.standard_normal(128 * 3)).astype(np.float32)      # a visible rotation, as in test_gpu_train_all._setup
    o, d = syn.sphere_rays(B, seed=seed)
    return table, torch.tensor(so3, dtype=F64), torch.tensor(o, dtype=F64), torch.tensor(d, dtype=F64)


def _march_record(table, so3, o, d, ndim, nmin, nmax, near, far, N, alpha):
    """TR.path_sampler_all's loop, recording what the device's march records: position and UNnormalised direction per node, and the list
    of (node, ray) pairs on the boundary shell (|g| > 1e-3) in (node, ray) order with their positions and looked-up gradients."""
    step = (far - near) / (N - 1)
    rp, rd = o + near * d, d.clone()
    pd, rdn, pair_of_node, px, pg = [], [], [], [], []
    n_pairs = 0
    with torch.no_grad():
        for _ in range(N):
            pd.append(rp); rdn.append(rd)
            n, g, pred = TR.vox_mlp_call_t(table, so3, rp, ndim, nmin, nmax, alpha)
            shell = torch.linalg.norm(g, dim=-1) > 1e-3
            ids = torch.full((rp.shape[0],), -1, dtype=torch.int64)
            ids[shell] = n_pairs + torch.arange(int(shell.sum()))
            n_pairs += int(shell.sum())
            pair_of_node.append(ids); px.append(rp[shell]); pg.append(g[shell])
            rp, rd = rp + step / n * rd, rd + step * torch.where(shell[:, None], pred, g)
    return torch.stack(pd), torch.stack(rdn), torch.stack(pair_of_node), torch.cat(px), torch.cat(pg), step


@pytest.mark.parametrize("ndim,nmin,nmax", [([12, 12, 12], [-1.5] * 3, [1.5] * 3), ([10, 12, 14], [-1.4, -1.5, -1.6], [1.5, 1.6, 1.4])])
def test_chained_references_equal_autograd_through_the_whole_march(ndim, nmin, nmax):
    B, N, near, far, alpha = 6, 10, 2.0, 6.0, 0.5
    table, so3, o, d = _scene(ndim, nmin, nmax, B)
    rng = np.random.default_rng(1)
    sample_of_node = torch.full((N,), -1, dtype=torch.int64)
    nodes = np.array([0, 2, 3, 5, 8, 9])
    sample_of_node[nodes] = torch.arange(len(nodes))
    a_pos = torch.tensor(rng.standard_normal((len(nodes), B, 3)), dtype=F64)
    a_dir = torch.tensor(rng.standard_normal((len(nodes), B, 3)), dtype=F64)

    # plain autograd through the whole path
    th = so3.clone().requires_grad_(True)
    ray_pos, ray_dir, _ = TR.path_sampler_all(o, d, table, th, ndim, nmin, nmax, near, far, N, alpha)
    loss = (a_pos.permute(1, 0, 2) * ray_pos[:, nodes]).sum() + (a_dir.permute(1, 0, 2) * ray_dir[:, nodes]).sum()
    want = torch.autograd.grad(loss, th)[0]

    # the chain of the four references
    pd, rdn, pair_of_node, px, pg, step = _march_record(table, so3, o, d, ndim, nmin, nmax, near, far, N, alpha)
    assert torch.equal(pd.permute(1, 0, 2), ray_pos.detach())
    n_pairs = px.shape[0]
    assert n_pairs >= 8 and int((pair_of_node < 0).sum()) >= 8             # nodes on and off the shell
    s = AR.so3_reference(so3, px, alpha, want_J=True)
    A, P = AR.pair_jacobian_reference(table, ndim, nmin, nmax, px, pg, s["raw"], s["J"])
    v = AR.adjoint_scan_reference(table, ndim, nmin, nmax, pd, rdn, pair_of_node, A, P, a_pos, a_dir, sample_of_node, step)
    got = AR.so3_reference(so3, px, alpha, cot=v)["dflat"]
    scale = float(want.abs().max())
    err = float((got - want).abs().max()) / scale
    print(f"{ndim}: {n_pairs} pairs, chained references vs autograd of the whole march: {err:.2e} of max |g| = {scale:.2e}")
    assert scale > 1e-6 and err < 1e-9


def test_reference_pieces_against_their_definitions():
    """so3_reference's J and dx are one Jacobian; nerfmlp_input_reference's gradients equal central differences of TR.nerf_mlp; the float32
    evaluation that sets the tolerances stays close to float64 and floor_and_tol never returns a tolerance beyond its ceiling."""
    rng = np.random.default_rng(2)
    so3 = torch.tensor(syn.init_mlp_flat(rng, TR.SO3_MLP_SHAPES, 0.05), dtype=F64)
    x = torch.tensor(rng.uniform(-1.5, 1.5, (17, 3)), dtype=F64)
    cot = torch.tensor(rng.standard_normal((17, 3)), dtype=F64)
    s = AR.so3_reference(so3, x, 0.35, cot=cot, want_J=True)
    assert float((torch.einsum("ij,ija->ia", cot, s["J"]) - s["dx"]).abs().max()) < 1e-12 * float(s["dx"].abs().max())
    assert s["min_pre"].shape == (17,) and float(s["min_pre"].min()) >= 0
    s32 = AR.so3_reference(so3.float(), x.float(), 0.35, cot=cot.float())
    floor, tol = AR.floor_and_tol(s["dx"], s32["dx"], 2e-5)
    assert 0 < floor < 2.5e-6 and tol == max(8 * floor, 1e-6)
    assert AR.floor_and_tol(s["dx"], s32["dx"] * 1.001, 2e-5)[1] == 2e-5          # a ceiling is never exceeded
    assert AR.floor_and_tol(s["dx"], s["dx"], 2e-5) == (0.0, 1e-6)

    flat = torch.tensor(syn.init_params_flat(12, fine=False, bias_scale=0.1)["coarse_mlp"], dtype=F64)
    pos = torch.tensor(rng.uniform(-1, 1, (5, 3)), dtype=F64)
    dirs = torch.tensor(R.safe_l2_normalize(rng.standard_normal((5, 3))), dtype=F64)
    c4 = torch.tensor(rng.standard_normal((5, 4)), dtype=F64)
    d_pos, d_dir, min_pre = AR.nerfmlp_input_reference(flat, pos, dirs, c4)
    f = lambda p, q: (c4 * TR.nerf_mlp(flat, TR.pos_enc_t(p, 10), TR.pos_enc_t(q, 4))).sum(-1)
    assert float(min_pre.min()) > 1e-6                      # no ReLU switches inside the difference quotient's +-1e-7
    h = 1e-7
    for a in range(3):
        e = torch.zeros(3, dtype=F64); e[a] = h
        for got, fd in ((d_pos[:, a], (f(pos + e, dirs) - f(pos - e, dirs)) / (2 * h)), (d_dir[:, a], (f(pos, dirs + e) - f(pos, dirs - e)) / (2 * h))):
            assert float((got - fd).abs().max()) < 1e-5 * float(got.abs().max() + 1.0)
