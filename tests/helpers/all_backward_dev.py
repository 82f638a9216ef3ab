"""Device-side plumbing shared by the tests that hold the stage-"all*" backward kernels to the float64 references of all_backward_ref.py
(tests/test_gpu_all_backward_kernels.py, tests/test_gpu_table_limits.py): tensor conversions, the run-twice check, the fp32-versus-float64
cell agreement of a point, the cotangents that turn the so3 dgrad into a Jacobian, and the comparison of a reverse scan."""
from __future__ import annotations

import numpy as np
import torch

import all_backward_ref as AR


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def D(t):
    return t.detach().cpu().double()


def pad4(a):
    return np.concatenate([a, np.zeros(a.shape[:-1] + (1,), a.dtype)], -1)


def rel(dev, ref):
    return float((D(dev) - ref).abs().max()) / float(ref.abs().max())


def twice(fn):
    """Run a kernel twice: identical bits (none of the five has atomics in its sums)."""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(x, y), "two runs of the same kernel on the same inputs differ"
    return a


def cells(p, a, f, ndim, nmin, nmax):
    """(i0, i1, t) of VoxMLP._linear3 along axis a in the float type f: np.float32 repeats the device's arithmetic (fp32 nmin and spacing,
    common.h: make_grid_params; IEEE subtract, divide, floor), np.float64 the reference's."""
    nd = (nmax[a] - nmin[a]) / (ndim[a] - 1.0)
    x = (p.astype(f) - f(nmin[a])) / f(nd)
    i = np.floor(x)
    return np.clip(i, 0, ndim[a] - 1), np.clip(i + 1, 0, ndim[a] - 1), x - i


def same_cells(pts64, ndim, nmin, nmax):
    """True where the device's fp32 corner indices of a point are the float64 reference's on all three axes: the interpolant's position
    gradient jumps from cell to cell, so a point within an fp32 rounding of a lattice plane has two legitimate answers."""
    ok = np.ones(pts64.shape[0], bool)
    for a in range(3):
        c32, c64 = cells(pts64[:, a].numpy(), a, np.float32, ndim, nmin, nmax), cells(pts64[:, a].numpy(), a, np.float64, ndim, nmin, nmax)
        ok &= (c32[0] == c64[0]) & (c32[1] == c64[1])
    return torch.from_numpy(ok)


def jacobian_cotangents(n):
    """[3 n, 4] unit cotangents, row j * n + i = e_j for point i: so3_backward on them returns d raw_j / d x of every point — exactly as
    train._all_stage_backward builds them."""
    eye = torch.zeros((3 * n, 4), dtype=torch.float32, device="cuda:0")
    for j in range(3):
        eye[j * n:(j + 1) * n, j] = 1.0
    return eye


def check_scan(tag, v, ref, ref32, inside, ceiling):
    """v [np, 4] of ops.march_adjoint against the float64 scan `ref` [>= np, 3]; `inside` marks the pairs the scanned nodes hold."""
    vd = D(v)
    nv = vd.shape[0]
    assert float(ref[nv:].abs().max() if ref.shape[0] > nv else 0.0) == 0.0
    m, ref, ref32 = inside[:nv], ref[:nv], ref32[:nv]
    assert float(vd[~m].abs().max() if bool((~m).any()) else 0.0) == 0.0, "a pair outside the scanned nodes was written"
    assert float(vd[:, 3].abs().max()) == 0.0
    if not bool(m.any()) or float(ref.abs().max()) == 0.0:
        assert float(vd.abs().max()) == 0.0 and float(ref.abs().max()) == 0.0
        print(f"march_adjoint {tag}: no pair with a cotangent among these nodes, v is exactly zero")
        return
    floor, tol = AR.floor_and_tol(ref, ref32, ceiling)
    err = rel(vd[:, :3], ref)
    print(f"march_adjoint {tag}: {int(m.sum())} pairs, v err {err:.2e} (fp32 floor {floor:.2e}, tol {tol:.2e}), max |v| {float(ref.abs().max()):.2e}")
    assert err < tol
