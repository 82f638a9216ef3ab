"""The consumers of the IoR table at tables of 2-4 GiB, at their size limits and on the smallest grids.

rnerf_march, rnerf_march_all, rnerf_march_all_train and rnerf_march_adjoint address the table with 32-bit byte offsets built from 24-bit
multiplies (csrc/march.hip, csrc/small_mlp.hip: `gather` / `load_b`); their launchers promise any table below 4 GiB whose multiplied strides
fit 24 bits and refuse the rest (csrc/common.h: grid_fits_march / grid_fits_u32).  The other consumers (grid_build_table, grid_query,
so3_query, so3_pair_jacobian) use 64-bit offsets.  Here every one of them runs on tables ABOVE 2^31 bytes, where bit 31 of an offset is set,
against the oracle fed a lazily evaluated table (tests/helpers/lazy_table.py, proven by tests/test_lazy_table_host.py), and the launchers
are called with grids they must refuse.

Shape A = (160, 1023, 1024), reference order only, box [-1.5, 1.5]^3:
    sb0 = 1023 * 1024 * 16 = 16 760 832 < 2^24 = 16 777 216; the table has 160 * sb0 = 2 681 733 120 bytes > 2^31 = 2 147 483 648;
    sa0 = 2 * sb0 >= 2^24: rnerf_march (which multiplies the index by sb in reference order) accepts it, the three so3 entry points
    (which multiply index >> 1 by sa) refuse it.
Shape B = (300, 510, 1024), both layouts:
    reference order: sb0 = 510 * 1024 * 16 = 8 355 840, sa0 = 16 711 680 < 2^24; bricks: sa0 = 255 * 512 * 128 = 16 711 680 < 2^24;
    the table has 2 506 752 000 bytes in either layout (all dimensions even: no padding).  Every consumer accepts it.
`test_the_shapes_are_what_the_comments_say` asserts this arithmetic from the Grid spec.

Device memory: only one shape is alive at a time (one module-scoped fixture, parametrised by shape; the refusals ask for its "none").
Peak: shape B, its grid (0.63 GB) beside both tables (2 x 2.51 GB) = 5.64 GB — torch.cuda.max_memory_allocated() of the whole module,
printed at the fixture's teardown, says 5.64 GB; the refusals' largest table of zeros is 4.31 GB, alone on the device.

Tolerances.  Everything without a transcendental is compared bit for bit.  march_all: the project's 2e-5 (test_march_all_stage), unless the
oracle's own fp32 march deviates from its float64 march by more than a quarter of that on this scene — then 8 x that deviation.  It does:
6.5e-6 to 8.1e-6 depending on the host's sgemm, so the bound is 5.2e-5 to 6.5e-5; the device's largest error is 9.5e-7.  pair Jacobians and
the reverse scan: all_backward_ref.floor_and_tol with test_gpu_all_backward_kernels' ceilings; measured A 1.9e-7 (tol 7.5e-6), P 1.5e-7
(tol 1.1e-6), v 1.6e-7 (tol 2.7e-6).  so3_query: test_so3_query's 2e-6 of the gradient magnitude; measured 1.4e-6 of a bound of 2.6e-6.
Coverage (asserted from the oracle's voxel indices before any comparison, printed): 85.9 % of shape A's nodes and 74.5 % / 74.9 % of shape
B's (reference order / bricks) gather a corner at or above 2^31 bytes; the last entry and entry 0 are gathered; the paths leave their
straight rays by up to 1.02.  With bit 31 of ONE corner's offset dropped in march.hip (an in-bounds read from the wrong address) test_march
fails on 94 % of the positions.  The module takes about 4 s.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import all_backward_ref as AR          # noqa: E402
import table_limits_scene as S          # noqa: E402
from all_backward_dev import D, T, check_scan, jacobian_cotangents, pad4, rel, same_cells, twice          # noqa: E402
from lazy_table import LazyTable          # noqa: E402
from oracle import ref_np as R, torch_ref as TR          # noqa: E402
from samplenerfro_amd import _lib, synthetic as syn          # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"
NMIN, NMAX, NEAR, FAR, N = S.NMIN, S.NMAX, S.NEAR, S.FAR, S.N_NODES
LAYOUTS = {"A": ("reference",), "B": ("reference", "bricks")}
ALPHA = 0.8
ADJ_CEIL = 5e-5                      # tests/test_gpu_all_backward_kernels.py: the scan's v
PATH_TOL = 2e-5                      # tests/test_gpu_parity.py: test_march_all_stage
VARIANTS = ((False, False), (True, False), (False, True), (True, True))
T0 = time.time()


def strides(dims, layout):
    """(sa0, sb0, table bytes) as csrc/common.h: make_grid_params derives them from a grid spec, restated."""
    dims = [int(v) for v in dims]
    if layout == "reference":
        sb0 = dims[1] * dims[2] * 16
        return 2 * sb0, sb0, sb0 * dims[0]
    bx, by, bz = [(d + 1) // 2 for d in dims]
    return by * bz * 128, 64, bx * by * bz * 128


def table_bytes(spec):
    nf = _lib.load().rnerf_grid_table_floats(C.byref(spec))
    assert nf > 0
    return 4 * nf


def so3_params(out_std):
    """tests/test_gpu_parity.py: _so3 — a trained-looking head on the default initialisation."""
    rng = np.random.default_rng(21)
    flat = syn.init_mlp_flat(rng, TR.SO3_MLP_SHAPES, 0.05)
    flat[-(128 * 3 + 3):-3] = (out_std * rng.standard_normal(128 * 3)).astype(F32)
    return flat, syn.flat_to_np_tree(flat, TR.SO3_MLP_SHAPES)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def same_bits(dev, ref, what):
    np.testing.assert_array_equal(bits(dev.cpu().numpy() if torch.is_tensor(dev) else dev), bits(ref), err_msg=what)


@pytest.fixture(scope="module")
def big(request):
    """The device tables of one big shape in every layout it is tested in, built on the device from the lazy field's 1-D profiles; freed
    before the next shape is built."""
    from samplenerfro_amd import ops
    name = request.param
    if name == "none":
        yield None
        return
    dims = S.SHAPES[name]
    lz, o, d, out, straight = S.oracle_march(name)
    specs = {k: _lib.Grid.make(dims, NMIN, NMAX, k) for k in LAYOUTS[name]}
    grid = lz.device_grid(DEV)
    assert grid.shape == tuple(dims) and grid.dtype == torch.float32
    tabs = {k: ops.grid_build_table(grid, specs[k]) for k in specs}
    torch.cuda.synchronize()
    del grid
    # the coverage conditions, from the oracle's own voxel indices, before any comparison
    pos, vox = out[0], out[5]
    for k in specs:
        cov = S.coverage(vox, pos, straight, dims, k)
        print(f"shape {name} {dims} {k}: {100 * cov['high_share']:.1f} % of the {vox.shape[0] * vox.shape[1]} nodes gather a corner at or above 2^31 bytes; "
              f"last entry gathered: {cov['last']}, entry 0 gathered: {cov['first']}; marched path leaves the straight ray by up to {cov['bend']:.3f}")
        assert cov["high_share"] >= 0.25 and cov["last"] and cov["first"] and cov["bend"] > 1e-3
    distinct = S.distinct_corner_share(lz, vox)
    print(f"shape {name}: {100 * distinct:.2f} % of the nodes in a proper cell gather eight different rows")
    assert distinct >= 0.99          # a wrong corner address must change the bits: the field is nowhere constant inside the box
    sc = dict(name=name, dims=dims, lz=lz, specs=specs, tabs=tabs, o=o, d=d, oracle=out, cache={})
    yield sc
    sc["cache"].clear(); tabs.clear(); sc.clear()
    torch.cuda.empty_cache()
    print(f"shape {name}: torch.cuda.max_memory_allocated() = {torch.cuda.max_memory_allocated() / 1e9:.2f} GB, "
          f"{time.time() - T0:.1f} s since the module was imported")


on_A_and_B = pytest.mark.parametrize("big", ["A", "B"], indirect=True)
on_B = pytest.mark.parametrize("big", ["B"], indirect=True)
on_none = pytest.mark.parametrize("big", ["none"], indirect=True)


@on_A_and_B
def test_the_shapes_are_what_the_comments_say(big):
    two24, two31, two32 = 1 << 24, 1 << 31, 1 << 32
    if big["name"] == "A":
        sa0, sb0, nbytes = strides(big["specs"]["reference"].dims, "reference")
        assert sb0 == 16760832 < two24 <= sa0 and nbytes == 2681733120 and two31 < nbytes < two32
        assert table_bytes(big["specs"]["reference"]) == nbytes == big["tabs"]["reference"].numel() * 4
    else:
        sa0, sb0, nbytes = strides(big["specs"]["reference"].dims, "reference")
        assert sb0 == 8355840 and sa0 == 16711680 < two24 and nbytes == 2506752000
        sa0, _, nbytes_b = strides(big["specs"]["bricks"].dims, "bricks")
        assert sa0 == 255 * 512 * 128 == 16711680 < two24 and nbytes_b == 2506752000 and two31 < nbytes < two32
        for k in ("reference", "bricks"):
            assert table_bytes(big["specs"][k]) == nbytes == big["tabs"][k].numel() * 4


# ---- a. the table's entries (rnerf_grid_build_table: 64-bit offsets) ---------------------------------------------------------------------
@on_A_and_B
def test_table_entries(big):
    dims, lz = big["dims"], big["lz"]
    total = dims[0] * dims[1] * dims[2]
    rng = np.random.default_rng(3)
    corners = [(x * dims[1] + y) * dims[2] + z for x in (0, dims[0] - 1) for y in (0, dims[1] - 1) for z in (0, dims[2] - 1)]
    flat = np.concatenate([rng.integers(0, total, 100000), np.array(corners), np.arange(total - 64, total)]).astype(np.int64)
    want = lz[flat]
    assert float(np.abs(want[:, 1:]).max()) > 1.0 and len(np.unique(want[:, 0])) > 10000
    x, y, z = flat // (dims[1] * dims[2]), (flat // dims[2]) % dims[1], flat % dims[2]
    for k, tab in big["tabs"].items():
        at = S.entry_of(x, y, z, dims, k)
        assert int(at.max()) == tab.shape[0] - 1 and float((16 * at >= 2 ** 31).mean()) > 0.10      # (the part above 2^31: 20 % of A, 14 % of B)
        same_bits(tab[torch.from_numpy(at).to(DEV)], want, f"table entries, {k}")


# ---- b. grid_query / so3_query (64-bit offsets) --------------------------------------------------------------------------------------------
@on_B
def test_grid_query_and_so3_query(big):
    from samplenerfro_amd import ops
    dims, lz = big["dims"], big["lz"]
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1.9, 1.9, (4096, 3)).astype(F32)                # inside and outside the box (clamp-to-edge)
    pts[2048:, 0] = rng.uniform(0.9, 1.9, 2048).astype(F32)            # half of them in the table's upper end
    pts[:8] = np.array([[sx, sy, sz] for sx in (-1.5, 1.5) for sy in (-1.5, 1.5) for sz in (-1.5, 1.5)], F32)
    pts[8:10] = [[-5, -5, -5], [5, 5, 5]]
    ref, ridx = R.linear3(lz, pts, list(dims), NMIN, NMAX, return_idx=True)
    flat, tree = so3_params(0.3)
    n, g, pred = R.vox_mlp_call(lz, tree, pts, list(dims), NMIN, NMAX, 1.0)
    for k in LAYOUTS["B"]:
        high = float((S.corner_bytes(ridx, dims, k).max(-1) >= 2 ** 31).mean())
        print(f"grid_query {k}: {100 * high:.1f} % of the points gather a corner at or above 2^31 bytes")
        assert high >= 0.25
        out, idx = ops.grid_query(big["tabs"][k], big["specs"][k], T(pts), want_idx=True)
        same_bits(idx, ridx, f"grid_query indices, {k}")
        same_bits(out, ref, f"grid_query values, {k}")
        out, gp = ops.so3_query(big["tabs"][k], big["specs"][k], T(flat), T(pts), 1.0)
        same_bits(out, ref, f"so3_query lookup, {k}")
        gp = gp.cpu().numpy()
        # test_gpu_parity.test_so3_query: fp32 MFMA chain vs numpy sgemm + libm sin/cos, 2e-6 of the gradient magnitude
        err = float(np.abs(gp - pred).max())
        print(f"so3_query {k}: pred_grad err {err:.2e} (tol {2e-6 * max(1.0, float(np.abs(g).max())):.2e})")
        assert err <= 2e-6 * max(1.0, float(np.abs(g).max()))
        assert float(np.abs(gp - g).max()) > 1e-3                       # and it does rotate


# ---- c. march (32-bit offsets; reference order multiplies by sb, bricks by sa) -----------------------------------------------------------
@on_A_and_B
def test_march(big):
    from samplenerfro_amd import ops
    pos, dirs, dist, n, g, vox = big["oracle"]
    o, d = T(big["o"]), T(big["d"])
    first = {}
    for k in big["tabs"]:
        for want_ior, want_vox in VARIANTS:
            pd, dr, ior, vx = ops.march(big["tabs"][k], big["specs"][k], o, d, NEAR, FAR, N, want_ior=want_ior, want_vox=want_vox)
            tag = f"shape {big['name']} {k} ior={want_ior} vox={want_vox}"
            assert (ior is not None) == want_ior and (vx is not None) == want_vox
            if want_vox:
                same_bits(vx.permute(1, 0, 2), vox, tag + ": voxel indices")
            same_bits(pd[..., :3].permute(1, 0, 2), pos, tag + ": positions")
            same_bits(pd[..., 3].T, dist, tag + ": distances")
            same_bits(dr[..., :3].permute(1, 0, 2), dirs, tag + ": directions")
            if want_ior:
                same_bits(ior[..., :1].permute(1, 0, 2), n, tag + ": n")
                same_bits(ior[..., 1:].permute(1, 0, 2), g, tag + ": grad n")
            if want_ior and want_vox:
                first.setdefault(k, (pd, dr, ior, vx))
    if len(first) == 2:
        for a, b in zip(first["reference"], first["bricks"]):
            assert torch.equal(a, b), "the bricked table gives other bits than the reference layout"


# ---- d. march_all / march_all_train ---------------------------------------------------------------------------------------------------------
def so3_oracle(big):
    """R.path_sampler with the so3 term in fp32 and in float64 through the lazy table, once: (fp32 outputs, their deviation from float64)."""
    if "so3_oracle" not in big["cache"]:
        _, tree = so3_params(0.1)
        args = (big["o"], big["d"], big["lz"], list(big["dims"]), NMIN, NMAX, NEAR, FAR, N)
        a32 = R.path_sampler(*args, so3_params=tree, annealed_alpha=ALPHA)
        a64 = R.path_sampler(*args, dtype=np.float64, so3_params=tree, annealed_alpha=ALPHA)
        big["cache"]["so3_oracle"] = (a32, max(float(np.abs(a32[i] - a64[i]).max()) for i in range(3)))
    return big["cache"]["so3_oracle"]


def train_record(big):
    from samplenerfro_amd import ops
    if "rec" not in big["cache"]:
        flat, _ = so3_params(0.1)
        big["cache"]["so3_d"] = T(flat)
        big["cache"]["rec"] = {k: ops.march_all_train(big["tabs"][k], big["specs"][k], big["cache"]["so3_d"], T(big["o"]), T(big["d"]), NEAR, FAR, N, ALPHA,
                                                      coherent=False) for k in big["tabs"]}
    return big["cache"]["rec"]


@on_B
def test_march_all(big):
    from samplenerfro_amd import ops
    (rp, rd, rt, _, _), dev64 = so3_oracle(big)
    tol = PATH_TOL if dev64 <= PATH_TOL / 4 else 8 * dev64
    print(f"march_all: the oracle's fp32 march deviates from its float64 march by {dev64:.2e} on this scene -> tolerance {tol:.2e}")
    assert float(np.abs(rp - big["oracle"][0]).max()) > 1e-3            # the so3 term matters in this scene
    rec = train_record(big)
    so3_d, o, d = big["cache"]["so3_d"], T(big["o"]), T(big["d"])
    outs = {}
    for k in big["tabs"]:
        for coherent in (False, True):      # True: the shell-coherent ray order, whose coarse pre-march is rnerf_march on the same table
            pd, dr, ior = ops.march_all(big["tabs"][k], big["specs"][k], so3_d, o, d, NEAR, FAR, N, ALPHA, want_ior=True, coherent=coherent)
            if k in outs:
                assert all(torch.equal(a, b) for a, b in zip(outs[k], (pd, dr, ior))), "the ray order changed a value"
            outs[k] = (pd, dr, ior)
        pd, dr, ior = outs[k]
        errs = [float(np.abs(pd[..., :3].permute(1, 0, 2).cpu().numpy() - rp).max()), float(np.abs(pd[..., 3].T.cpu().numpy() - rt).max()),
                float(np.abs(dr[..., :3].permute(1, 0, 2).cpu().numpy() - rd).max())]
        print(f"march_all {k}: position / distance / direction err {errs[0]:.2e} / {errs[1]:.2e} / {errs[2]:.2e} (tol {tol:.2e})")
        assert max(errs) < tol
        assert torch.equal(rec[k]["path_pd"], pd) and torch.equal(rec[k]["path_dr"], dr), "march_all_train records another path than march_all"
        assert torch.equal(rec[k]["path_rdn"][..., 3], ior[..., 0])
    for a, b in zip(outs["reference"], outs["bricks"]):
        assert torch.equal(a, b), "the bricked table gives other bits than the reference layout"
    a, b = rec["reference"], rec["bricks"]
    assert a["n_pairs"] == b["n_pairs"] > 0
    for key in ("path_rdn", "pair_of_node", "pair_id", "pair_x", "pair_g"):
        assert torch.equal(a[key], b[key]), key


# ---- e. so3_pair_jacobian (64-bit offsets) / march_adjoint (32-bit offsets) on the record of d --------------------------------------------
N_LAST, B_ADJ = 32, 32


@on_B
def test_pair_jacobian_and_march_adjoint(big):
    from samplenerfro_amd import ops
    dims, lz64 = list(big["dims"]), big["lz"].torch_face()
    rec = train_record(big)["reference"]
    so3_d = big["cache"]["so3_d"]
    lo = N - N_LAST
    pon = rec["pair_of_node"][lo:].cpu()
    share_all = float((rec["pair_of_node"] >= 0).float().mean())
    print(f"boundary-shell pairs: {100 * share_all:.1f} % of the record's nodes")
    assert 0.02 < share_all < 0.5
    # rays: those with pairs among the last N_LAST nodes, filled up with rays without; a ray any of whose scanned nodes lies within an fp32
    # rounding of a lattice plane (two legitimate cells, all_backward_dev.same_cells) is left out before anything runs
    has = (pon >= 0).any(0)
    cand = torch.cat([torch.nonzero(has)[:, 0], torch.nonzero(~has)[:, 0]])
    pts = D(rec["path_pd"][lo:])[..., :3]
    ok = torch.stack([same_cells(pts[:, r], dims, NMIN, NMAX).all() for r in cand.tolist()])
    left_out = 1.0 - float(ok.double().mean())
    print(f"{100 * left_out:.1f} % of the rays have a node within an fp32 rounding of a lattice plane")
    assert left_out <= 0.10
    sel = cand[ok][:B_ADJ].sort().values
    assert sel.numel() == B_ADJ and int(has[sel].sum()) >= 12
    sel_d = sel.to(DEV)
    pon_sub = rec["pair_of_node"][lo:][:, sel_d].contiguous()
    m = pon_sub >= 0
    old = pon_sub[m].long()
    n = int(old.numel())
    print(f"{B_ADJ} rays x {N_LAST} nodes: {n} pairs ({100 * n / (B_ADJ * N_LAST):.1f} % of the scanned nodes)")
    assert n > 100 and n < 0.5 * B_ADJ * N_LAST
    pon_new = torch.full_like(pon_sub, -1)
    pon_new[m] = torch.arange(n, dtype=torch.int32, device=DEV)
    pair_x, pair_g = rec["pair_x"][old].contiguous(), rec["pair_g"][old].contiguous()
    high = float((S.corner_bytes(R.linear3(big["lz"], pair_x[:, :3].cpu().numpy(), dims, NMIN, NMAX, return_idx=True)[1], dims, "reference").max(-1) >= 2 ** 31).mean())
    print(f"{100 * high:.1f} % of the pairs gather a corner at or above 2^31 bytes")
    assert high >= 0.25
    raw, save = ops.so3_forward_train(so3_d, rec["window"], pair_x)
    J = ops.so3_backward(so3_d, rec["window"], pair_x, save, jacobian_cotangents(n))
    raw = raw.contiguous()
    AP = {k: twice(lambda: tuple(m[:, :9] for m in ops.so3_pair_jacobian(big["tabs"][k], big["specs"][k], pair_x, pair_g, raw, J)))
          for k in big["tabs"]}                                          # 12 floats per pair, 9 used
    assert torch.equal(AP["bricks"][0], AP["reference"][0]) and torch.equal(AP["bricks"][1], AP["reference"][1]), "the bricked table gives other bits"
    A, P = (torch.cat([m, torch.zeros((n, 3), dtype=torch.float32, device=DEV)], 1) for m in AP["reference"])
    args = (D(pair_x)[:, :3], D(pair_g)[:, :3], D(raw)[:, :3], D(J)[:, :3].reshape(3, n, 3).permute(1, 0, 2).contiguous())
    ref = AR.pair_jacobian_reference(lz64, dims, NMIN, NMAX, *args)
    ref32 = AR.pair_jacobian_reference(lz64.float(), dims, NMIN, NMAX, *(t.float() for t in args))
    for name, dev, r64, r32 in (("A", A, ref[0], ref32[0]), ("P", P, ref[1], ref32[1])):
        floor, tol = AR.floor_and_tol(r64, r32)
        err = rel(dev[:, :9].reshape(n, 3, 3), r64)
        print(f"pair_jacobian {name}: err {err:.2e} (fp32 floor {floor:.2e}, tol {tol:.2e}), max |{name}| {float(r64.abs().max()):.2e}")
        assert err < tol
    # the reverse scan over the last N_LAST nodes (the recurrence is self-consistent from any node), every third node a sample, the last among them
    rng = np.random.default_rng(41)
    son = np.full(N_LAST, -1, np.int32)
    son[(N_LAST - 1) % 3::3] = np.arange(len(son[(N_LAST - 1) % 3::3]))
    n_s = int(son.max()) + 1
    assert son[-1] == n_s - 1
    a_pos, a_dir = T(pad4(rng.standard_normal((n_s, B_ADJ, 3)).astype(F32))), T(pad4(rng.standard_normal((n_s, B_ADJ, 3)).astype(F32)))
    step = (FAR - NEAR) / (N - 1)
    far = NEAR + step * (N_LAST - 1)                                  # the same step for the shorter scan
    sub = dict(path_pd=rec["path_pd"][lo:][:, sel_d].contiguous(), path_rdn=rec["path_rdn"][lo:][:, sel_d].contiguous(), pair_of_node=pon_new, n_pairs=n)
    assert int(pon_new.max()) == n - 1 < A.shape[0]
    v = {k: twice(lambda: ops.march_adjoint(big["tabs"][k], big["specs"][k], sub, A, P, a_pos, a_dir, T(son), NEAR, far)) for k in big["tabs"]}
    assert torch.equal(v["reference"], v["bricks"]), "the bricked table gives other bits than the reference layout"
    son64 = torch.from_numpy(son.astype(np.int64))
    args = [D(sub["path_pd"]), D(sub["path_rdn"]), pon_new.cpu().long(), D(A)[:, :9].reshape(-1, 3, 3), D(P)[:, :9].reshape(-1, 3, 3), D(a_pos), D(a_dir)]
    ref = AR.adjoint_scan_reference(lz64, dims, NMIN, NMAX, *args, son64, step)
    ref32 = AR.adjoint_scan_reference(lz64.float(), dims, NMIN, NMAX, args[0].float(), args[1].float(), args[2], *(t.float() for t in args[3:]), son64, step)
    check_scan(f"shape B, last {N_LAST} nodes of {B_ADJ} rays", v["reference"], ref, ref32, torch.ones(n, dtype=torch.bool), ADJ_CEIL)


# ---- f. refusals ----------------------------------------------------------------------------------------------------------------------------
SMALL = (2, 3, 5)


def small_scene():
    rng = np.random.default_rng(0)
    lz = LazyTable(*[rng.uniform(-0.2, 0.6, n).astype(F32) for n in SMALL], SMALL, NMIN, NMAX)
    o, d = syn.sphere_rays(20, seed=3)
    return lz, o, d


def the_four(table, spec, so3_d, o, d, n_nodes=8):
    """name -> call of the four 32-bit consumers on `table`; the adjoint scans a record of zeros without pairs."""
    from samplenerfro_amd import ops
    B = o.shape[0]
    z4 = lambda *s: torch.zeros(s + (4,), dtype=torch.float32, device=DEV)
    rec = dict(path_pd=z4(n_nodes, B), path_rdn=z4(n_nodes, B), pair_of_node=torch.full((n_nodes, B), -1, dtype=torch.int32, device=DEV), n_pairs=0)
    son = torch.full((n_nodes,), -1, dtype=torch.int32, device=DEV)
    return {"march": lambda: ops.march(table, spec, o, d, NEAR, FAR, n_nodes, want_ior=True, want_vox=True),
            "march_all": lambda: ops.march_all(table, spec, so3_d, o, d, NEAR, FAR, n_nodes, ALPHA, want_ior=True, coherent=False),
            "march_all_train": lambda: ops.march_all_train(table, spec, so3_d, o, d, NEAR, FAR, n_nodes, ALPHA, coherent=False)["path_pd"],
            "march_adjoint": lambda: ops.march_adjoint(table, spec, rec, z4(3).view(1, 12), z4(3).view(1, 12), z4(1, B), z4(1, B), son, NEAR, FAR)}


REFUSALS = [((160, 1023, 1024), "reference", ("march",)),                     # shape A: sb0 < 2^24 <= sa0
            ((300, 512, 1024), "reference", ("march",)),                      # sa0 = 2^24 exactly, sb0 = 2^23
            ((300, 512, 1024), "bricks", ()),                                 # sa0 = 256 * 512 * 128 = 2^24 exactly
            ((257, 1023, 1024), "reference", ())]                             # 24-bit strides, 4 307 533 824 bytes >= 2^32


@on_none
@pytest.mark.parametrize("dims,layout,accepted", REFUSALS)
def test_refusals(big, dims, layout, accepted):
    from samplenerfro_amd import ops
    sa0, sb0, nbytes = strides(dims, layout)
    mult = sb0 if layout == "reference" else sa0                     # what rnerf_march multiplies an index by
    fits_march, fits_so3 = nbytes < 2 ** 32 and mult < 2 ** 24, nbytes < 2 ** 32 and sa0 < 2 ** 24
    assert fits_march == ("march" in accepted) and not fits_so3      # the cases are what their comments say
    flat, _ = so3_params(0.1)
    so3_d = T(flat)
    lz, o, d = small_scene()
    o, d = T(o), T(d)
    sspec = _lib.Grid.make(SMALL, NMIN, NMAX, layout)
    stab = ops.grid_build_table(T(lz.dense_grid()), sspec)
    small = the_four(stab, sspec, so3_d, o, d)
    base = {k: fn() for k, fn in small.items()}
    spec = _lib.Grid.make(dims, NMIN, NMAX, layout)
    assert table_bytes(spec) == nbytes
    table = torch.zeros((nbytes // 16, 4), dtype=torch.float32, device=DEV)      # real memory of the full size: a broken check still reads inside it
    calls = the_four(table, spec, so3_d, o, d)
    for name in ("march_all", "march_all_train", "march_adjoint", "march"):
        if name in accepted:
            continue
        with pytest.raises(_lib.RnerfError, match="grid too large"):
            calls[name]()
        again = small[name]()                                         # the error left nothing behind
        for a, b in zip(base[name] if isinstance(base[name], tuple) else (base[name],), again if isinstance(again, tuple) else (again,)):
            assert torch.equal(a, b), f"{name} on a small grid changed after the refusal"
    if "march" in accepted:
        table[:, 0] = 1.0                                             # vacuum: n = 1, grad n = 0 -> straight rays
        vac = LazyTable(*[np.zeros(n, F32) for n in dims], dims, NMIN, NMAX)
        pos, dirs, dist, n, g, vox = R.path_sampler(o.cpu().numpy(), d.cpu().numpy(), vac, list(dims), NMIN, NMAX, NEAR, FAR, 8, return_idx=True)
        pd, dr, ior, vx = calls["march"]()
        same_bits(vx.permute(1, 0, 2), vox, "vacuum march: voxel indices")
        same_bits(pd[..., :3].permute(1, 0, 2), pos, "vacuum march: positions")
        same_bits(ior[..., :1].permute(1, 0, 2), n, "vacuum march: n")
    del table, calls
    torch.cuda.empty_cache()


# ---- g. the smallest grids ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 3, 5), (3, 2, 2)])
def test_smallest_grids(dims):
    from samplenerfro_amd import ops
    nmin, nmax = [-1.5, -1.0, -0.5], [1.4, 1.2, 0.9]
    rng = np.random.default_rng(sum(dims))
    lz = LazyTable(*[rng.uniform(-0.2, 0.6, n).astype(F32) for n in dims], dims, nmin, nmax)
    grid = lz.dense_grid()
    table = R.build_table(grid, list(dims), nmin, nmax)
    o = (4.0 * R.safe_l2_normalize(rng.standard_normal((37, 3)).astype(F32))).astype(F32)
    centre = 0.5 * (np.array(nmin) + np.array(nmax))
    d = R.safe_l2_normalize((centre + 0.5 * (rng.uniform(nmin, nmax, (37, 3)) - centre) - o).astype(F32))      # aimed at the box's inner half
    n_nodes = 50
    pos, dirs, dist, n, g, vox = R.path_sampler(o, d, table, list(dims), nmin, nmax, NEAR, FAR, n_nodes, return_idx=True)
    inside = np.all((pos >= np.array(nmin, F32)) & (pos <= np.array(nmax, F32)), -1)
    # the rays cross the box (the edge rows' gradient reaches beyond it and bends a few of them away), with nodes on both sides of its faces
    assert float(inside.any(1).mean()) > 0.75 and 0.25 < float(inside.mean()) < 0.9 and float(np.abs(g).max()) > 1e-2
    pts = rng.uniform(-1.9, 1.9, (512, 3)).astype(F32)
    pts[:2] = [nmin, nmax]
    ref, ridx = R.linear3(table, pts, list(dims), nmin, nmax, return_idx=True)
    flat, tree = so3_params(0.1)
    for k in ("reference", "bricks"):
        spec = _lib.Grid.make(dims, nmin, nmax, k)
        tab = ops.grid_build_table(T(grid), spec)
        out, idx = ops.grid_query(tab, spec, T(pts), want_idx=True)
        same_bits(idx, ridx, f"{dims} {k}: grid_query indices")
        same_bits(out, ref, f"{dims} {k}: grid_query values")
        for want_ior, want_vox in VARIANTS:
            pd, dr, ior, vx = ops.march(tab, spec, T(o), T(d), NEAR, FAR, n_nodes, want_ior=want_ior, want_vox=want_vox)
            tag = f"{dims} {k} ior={want_ior} vox={want_vox}"
            same_bits(pd[..., :3].permute(1, 0, 2), pos, tag + ": positions")
            same_bits(pd[..., 3].T, dist, tag + ": distances")
            same_bits(dr[..., :3].permute(1, 0, 2), dirs, tag + ": directions")
            if want_ior:
                same_bits(ior[..., :1].permute(1, 0, 2), n, tag + ": n")
                same_bits(ior[..., 1:].permute(1, 0, 2), g, tag + ": grad n")
            if want_vox:
                same_bits(vx.permute(1, 0, 2), vox, tag + ": voxel indices")
    if dims == (2, 3, 5):
        rp, rd, rt, _, _ = R.path_sampler(o, d, table, list(dims), nmin, nmax, NEAR, FAR, n_nodes, so3_params=tree, annealed_alpha=ALPHA)
        assert float(np.abs(rp - pos).max()) > 1e-3                    # the so3 term matters
        outs = {}
        for k in ("reference", "bricks"):
            spec = _lib.Grid.make(dims, nmin, nmax, k)
            tab = ops.grid_build_table(T(grid), spec)
            pd, dr, _ = outs[k] = ops.march_all(tab, spec, T(flat), T(o), T(d), NEAR, FAR, n_nodes, ALPHA)
            errs = [float(np.abs(pd[..., :3].permute(1, 0, 2).cpu().numpy() - rp).max()), float(np.abs(pd[..., 3].T.cpu().numpy() - rt).max()),
                    float(np.abs(dr[..., :3].permute(1, 0, 2).cpu().numpy() - rd).max())]
            print(f"march_all {dims} {k}: position / distance / direction err {errs[0]:.2e} / {errs[1]:.2e} / {errs[2]:.2e} (tol {PATH_TOL:.1e})")
            assert max(errs) < PATH_TOL                                # test_gpu_parity.test_march_all_stage
        assert torch.equal(outs["reference"][0], outs["bricks"][0]) and torch.equal(outs["reference"][1], outs["bricks"][1])
