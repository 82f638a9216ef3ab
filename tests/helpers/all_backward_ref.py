"""References for the five stage-"all*" backward kernels (csrc/small_mlp.hip; the input gradient: csrc/mlp.hip), in torch on the CPU (TEST INFRASTRUCTURE, no device).

Each reference states ONE kernel's operation, on the inputs that kernel was given, from the pieces of oracle/torch_ref.py and torch.autograd —
none repeats the kernels' hand-derived formulas.  Every function computes in the dtype of its tensor arguments: float64 is the reference,
the same call on float32 copies gives the noise floor of plain fp32 arithmetic (`floor_and_tol`).  tests/test_all_backward_ref_host.py
chains the four of them and compares with autograd through the whole march (TR.path_sampler_all).
"""
from __future__ import annotations

import torch

from oracle import torch_ref as TR


def _layers(flat, shapes):
    ps, off = [], 0
    for i, o in shapes:
        ps.append((flat[off:off + i * o].view(i, o), flat[off + i * o:off + i * o + o]))
        off += i * o + o
    return ps


def so3_preactivations(flat, enc):
    """The forward loop of TR.so3_mlp restated to expose the four ReLU layers' pre-activations -> (raw [n,3], [z_0 .. z_3])."""
    ps = _layers(flat, TR.SO3_MLP_SHAPES)
    h, pre = enc, []
    for i in range(4):
        z = h @ ps[i][0] + ps[i][1]
        pre.append(z)
        h = torch.relu(z)
        if i == 2:
            h = torch.cat([h, enc], -1)
    return h @ ps[4][0] + ps[4][1], pre


def so3_reference(flat, x, alpha, cot=None, want_J=False):
    """so3_mlp(annealed_pos_enc(x, alpha * 10)) at x [n,3] -> dict:
    raw [n,3]; min_pre [n] = the smallest |pre-activation| of the row over the four ReLU layers; with cot [n,3]: dx [n,3] and dflat, the
    gradients of sum(cot * raw); with want_J: J [n,3,3], J[i,j] = d raw_j / d x of point i, one autograd pass per j."""
    flat = flat.detach().clone().requires_grad_(True)
    x = x.detach().clone().requires_grad_(True)
    enc = TR.annealed_pos_enc_t(x, alpha * 10.0)
    raw = TR.so3_mlp(flat, enc)
    with torch.no_grad():
        raw2, pre = so3_preactivations(flat, enc)
        assert torch.equal(raw2, raw)
        min_pre = torch.stack([z.abs().min(-1)[0] for z in pre], 0).min(0)[0]
    out = {"raw": raw.detach(), "min_pre": min_pre}
    if cot is not None:
        out["dx"], out["dflat"] = torch.autograd.grad((cot * raw).sum(), (x, flat), retain_graph=want_J)
    if want_J:
        out["J"] = torch.stack([torch.autograd.grad(raw[:, j].sum(), x, retain_graph=j < 2)[0] for j in range(3)], 1)
    return out


def nerfmlp_input_reference(flat, pos, dirs, cot):
    """d / d pos, d / d dirs [R,3] of sum(cot * TR.nerf_mlp(flat, pos_enc(pos, 10), pos_enc(dirs, 4))), cot [R,4], and per row the smallest
    |pre-activation| over the 8 trunk layers and the view layer."""
    pos = pos.detach().clone().requires_grad_(True)
    dirs = dirs.detach().clone().requires_grad_(True)
    x, cond = TR.pos_enc_t(pos, 10), TR.pos_enc_t(dirs, 4)
    raw = TR.nerf_mlp(flat, x, cond)
    d_pos, d_dir = torch.autograd.grad((cot * raw).sum(), (pos, dirs))
    with torch.no_grad():      # TR.nerf_mlp's loop again, for the pre-activations
        ps = _layers(flat, TR.NERF_MLP_SHAPES)
        h, pre = x, []
        for i in range(8):
            z = h @ ps[i][0] + ps[i][1]
            pre.append(z)
            h = torch.relu(z)
            if i == 4:
                h = torch.cat([h, x], -1)
        sigma = h @ ps[8][0] + ps[8][1]
        zv = torch.cat([h @ ps[9][0] + ps[9][1], cond], -1) @ ps[10][0] + ps[10][1]
        pre.append(zv)
        assert torch.equal(torch.cat([torch.relu(zv) @ ps[11][0] + ps[11][1], sigma], -1), raw)
        min_pre = torch.stack([z.abs().min(-1)[0] for z in pre], 0).min(0)[0]
    return d_pos, d_dir, min_pre


def rodrigues_t(raw, g):
    """pred of TR.vox_mlp_call_t as a function of the so3 output and the looked-up gradient (both norms clamped as in TR.safe_norm_t)."""
    theta = TR.safe_norm_t(raw)
    e = raw / theta
    a = TR.safe_norm_t(g)
    v = g / a
    return a * (torch.cos(theta) * v + torch.sin(theta) * torch.cross(e, v, dim=-1) + (1 - torch.cos(theta)) * (e * v).sum(-1, keepdim=True) * e)


def _rowwise_jacobian(fn, x):
    """[n,3,3]: out[i, c, a] = d fn(x)[i, c] / d x[i, a] of a function that acts on every row on its own."""
    x = x.detach().clone().requires_grad_(True)
    y = fn(x)
    return torch.stack([torch.autograd.grad(y[:, c].sum(), x, retain_graph=c < 2)[0] for c in range(3)], 1)


def pair_jacobian_reference(table, ndim, nmin, nmax, x, g, raw, J):
    """x, g, raw [n,3], J [n,3,3] (J[i,j] = d raw_j / d x) -> (A, P) [n,3,3]: P = d pred / d raw and A = P J + (d pred / d g) G of the rotated
    gradient pred = Rodrigues(raw, g), with G = d g / d x of the trilinear interpolant TR.linear3_t."""
    P = _rowwise_jacobian(lambda r: rodrigues_t(r, g), raw)
    Q = _rowwise_jacobian(lambda gg: rodrigues_t(raw, gg), g)
    G = _rowwise_jacobian(lambda p: TR.linear3_t(table, p, ndim, nmin, nmax)[:, 1:], x)
    return P @ J + Q @ G, P


def adjoint_scan_reference(table, ndim, nmin, nmax, path_pd, path_rdn, pair_of_node, A, P, a_pos, a_dir, sample_of_node, step):
    """The reverse scan of the march with autograd for every per-node vector-Jacobian product.  path_pd, path_rdn [N,B,>=3] (recorded
    position, UNnormalised direction), pair_of_node [N,B] (index into A, P [np,3,3], -1 off the shell), a_pos, a_dir [S,B,>=3] (cotangents of
    the position and of the safe-normalised direction of the samples), sample_of_node [N] (-1: no sample) -> v [np,3], the cotangent of the
    so3 output at every pair the scan meets (zeros elsewhere).
    One step of the recurrence: p' = p + step / n(p) d, d' = d + step grad(p); grad = g(p) off the shell, and on it the pair's linearisation
    A (p - p0) + P delta in the position and in a perturbation delta of the so3 output."""
    N, B = pair_of_node.shape
    dt = path_pd.dtype
    lp = torch.zeros((B, 3), dtype=dt)
    ld = torch.zeros((B, 3), dtype=dt)
    v = torch.zeros((A.shape[0], 3), dtype=dt)
    for k in range(N - 1, -1, -1):
        p = path_pd[k, :, :3].detach().clone().requires_grad_(True)
        d = path_rdn[k, :, :3].detach().clone().requires_grad_(True)
        delta = torch.zeros((B, 3), dtype=dt, requires_grad=True)
        ng = TR.linear3_t(table, p, ndim, nmin, nmax)
        n, g = ng[:, :1], ng[:, 1:]
        pr = pair_of_node[k].long()
        is_pair = pr >= 0
        idx = pr.clamp(min=0)
        lin = (A[idx] @ (p - p.detach())[..., None] + P[idx] @ delta[..., None])[..., 0]
        grad = torch.where(is_pair[:, None], lin, g)
        obj = (lp * (p + step / n * d)).sum() + (ld * (d + step * grad)).sum()
        s = int(sample_of_node[k])
        if s >= 0:
            obj = obj + (a_pos[s, :, :3] * p).sum() + (a_dir[s, :, :3] * (d / TR.safe_norm_t(d))).sum()
        lp, ld, vk = torch.autograd.grad(obj, (p, d, delta))
        v[idx[is_pair]] = vk[is_pair]
    return v


def floor_and_tol(ref64, ref32, ceiling=None):
    """The tolerance of a kernel that computes in plain fp32: 8 x the largest deviation of the SAME reference evaluated in float32 from its
    float64 result, relative to the tensor's largest magnitude (8: another association of the same fp32 sums), at least 1e-6 — and never
    more than `ceiling`, the bound the project already holds this arithmetic to: where 8 x the floor exceeds it, the ceiling is the bound.
    -> (floor, tolerance)."""
    scale = float(ref64.abs().max())
    assert scale > 0
    floor = float((ref32.double() - ref64).abs().max()) / scale
    tol = max(8.0 * floor, 1e-6)
    return floor, tol if ceiling is None else min(tol, ceiling)
