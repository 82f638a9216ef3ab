"""The dgrad across its tile seam: one launch whose workgroup 0 runs two tiles against the same rows as two one-tile-per-workgroup launches.

65 755 rows are 257 tiles of 256 rows: on 256 CUs the persistent dgrad gives workgroup 0 a second tile (whatever it prefetches or keeps
for "the next tile" is then live), and that last tile is padded (rows 65 755 .. 65 791 do not exist).  The same rows as two launches,
33 024 rows (129 full tiles: too many for 128-row tiles, one 256-row tile per workgroup) and the remaining 32 731 (128 tiles: the 128-row
variant where the mode has one, 256 workgroups of one tile each), never cross a tile seam.  A row's arithmetic does not depend on the tile
or the launch it sits in, so every dY plane and every row scale must be IDENTICAL row for row (the padded rows included: both record the
zero gradient), and the launch's m_ref, the largest row scale, must be the larger of the two parts'.  A 256-row launch (a single tile, run
as two 128-row tiles) must give the bits of the first 256 rows again.

d raw has a few all-zero rows (row scale 0: they contribute nothing) and one row 1000 x the others (it alone sets m_ref).
"""
import numpy as np
import pytest

ROWS, PART_A, ONE_TILE = 65755, 33024, 256          # 257 tiles; 129 full tiles + 128 tiles (the last one ragged); one tile
DY_SLOTS = 153                                      # csrc/mlp.hip: slots per 32-row tile of a dY plane
ZERO_ROWS = (0, 77, 255, 256, 33023, 33024, 50000, 65754)
BIG_ROW = 40001                                     # in the second part and in a tile of workgroup 144, not the seam-crossing one
MODES = ("f32", "f16x3lo8", "tf32", "bf16")


def _padded(rows):
    return (rows + 255) // 256 * 256


@pytest.fixture(scope="module")
def inputs():
    import torch
    from samplenerfro_amd import _lib, ops, synthetic as syn
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(2024)
    pos = rng.uniform(-3, 3, (ROWS, 3)).astype(np.float32)
    d = rng.standard_normal((ROWS, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = rng.uniform(2, 6, (ROWS, 1)).astype(np.float32)
    d_raw = (rng.standard_normal((ROWS, 4)) * 1e-3).astype(np.float32)
    d_raw[list(ZERO_ROWS)] = 0.0
    d_raw[BIG_ROW] *= 1000.0
    pf = T(syn.init_params_flat(7, bias_scale=0.1)["coarse_mlp"])
    P = _lib.PRECISIONS["f16x3"]
    return {"pd": T(np.concatenate([pos, t], -1)), "dr": T(np.concatenate([d, np.zeros((ROWS, 1), np.float32)], -1)), "d_raw": T(d_raw),
            "pf": pf, "P": P, "packed": ops.nerfmlp_pack(pf, P)}


def _dgrad(inp, mode, lo, hi):
    """Training forward + dgrad of rows [lo, hi) as one launch each -> (dY planes as [plane][32-row tile] bytes, row scales, m_ref)."""
    import torch
    from samplenerfro_amd import _lib, ops
    BW = _lib.BACKWARDS[mode]
    n = hi - lo
    R = _padded(n)
    pd, dr, d_raw = (inp[k][lo:hi].contiguous().reshape(1, n, 4) for k in ("pd", "dr", "d_raw"))
    _, save = ops.nerfmlp_forward_train(inp["packed"], inp["P"], pd, dr, None, 1, n, BW)
    pbwd = ops.nerfmlp_pack_bwd(inp["pf"], None, BW)
    dy = torch.full((_lib.load().rnerf_nerfmlp_dy_bytes(n, BW),), 0xA5, dtype=torch.uint8, device=pd.device)
    ops.nerfmlp_backward(pbwd, inp["packed"], inp["P"], save, d_raw, n, dy=dy, stages="d", backward=BW)
    torch.cuda.synchronize()
    plane = DY_SLOTS * R * 2 * 16                    # bytes of one uint4 plane: [32-row tile][slot][row in tile][half]
    planes = [dy[:plane].view(R // 32, -1)]
    if BW in _lib.TWO_PLANE_BACKWARDS:               # the lo plane: uint4 again, or e4m3 bytes (uint2) at the head of its place
        lo_bytes = plane // 2 if BW == _lib.BWD_F16X3_LO8 else plane
        planes.append(dy[plane:plane + lo_bytes].view(R // 32, -1))
    if mode == "bf16":                               # no row normalisation: neither row scales nor m_ref
        return planes, None, None
    tail = dy[plane * (2 if BW in _lib.TWO_PLANE_BACKWARDS else 1):].view(torch.float32)
    assert tail.numel() == R + 4
    return planes, tail[:R], tail[R:R + 1]


@pytest.fixture(scope="module")
def runs(inputs):
    cache = {}

    def get(mode, lo, hi):
        if (mode, lo, hi) not in cache:
            cache[(mode, lo, hi)] = _dgrad(inputs, mode, lo, hi)
        return cache[(mode, lo, hi)]
    return get


def _same_bytes(a, b, what):
    import torch
    assert a.shape == b.shape, what
    if not torch.equal(a, b):
        bad = (a != b).any(dim=-1).nonzero().flatten()
        raise AssertionError(f"{what}: {bad.numel()} of {a.shape[0]} 32-row tiles differ, first {bad[:8].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_two_tiles_per_workgroup_give_the_bits_of_one_tile_per_workgroup(runs, mode):
    import torch
    whole, part_a, part_b = runs(mode, 0, ROWS), runs(mode, 0, PART_A), runs(mode, PART_A, ROWS)
    ta = PART_A // 32
    assert len(whole[0]) == len(part_a[0]) == len(part_b[0]) == (2 if mode in ("f32", "f16x3lo8") else 1)
    for p, (w, a, b) in enumerate(zip(whole[0], part_a[0], part_b[0])):
        assert w.shape[0] == a.shape[0] + b.shape[0] == _padded(ROWS) // 32
        _same_bytes(w[:ta], a, f"{mode}: dY plane {p}, rows of the first part")
        _same_bytes(w[ta:], b, f"{mode}: dY plane {p}, rows of the second part")
    if mode == "bf16":
        return
    bits = lambda x: x.view(torch.int32)
    rs = bits(whole[1])
    assert torch.equal(rs[:PART_A], bits(part_a[1])) and torch.equal(rs[PART_A:], bits(part_b[1])), f"{mode}: row scales differ"
    scales = whole[1].cpu().numpy()
    assert (scales[list(ZERO_ROWS)] == 0).all() and (scales[ROWS:] == 0).all() and (np.delete(scales[:ROWS], list(ZERO_ROWS)) > 0).all()
    m = [float(x[2].item()) for x in (whole, part_a, part_b)]
    print(f"{mode}: m_ref whole {m[0]!r}, parts {m[1]!r} {m[2]!r}")
    assert m[0] == max(m[1], m[2]) and m[2] > m[1] > 0                     # the big row sits in the second part
    assert m[0] == float(scales.max()) == float(scales[BIG_ROW])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_single_tile_gives_the_bits_of_its_rows_in_the_large_launch(runs, mode):
    import torch
    whole, one = runs(mode, 0, ROWS), runs(mode, 0, ONE_TILE)
    for p, (w, o) in enumerate(zip(whole[0], one[0])):
        assert o.shape[0] == ONE_TILE // 32
        _same_bytes(w[:ONE_TILE // 32], o, f"{mode}: dY plane {p} of the single tile")
    if mode == "bf16":
        return
    assert torch.equal(whole[1][:ONE_TILE].view(torch.int32), one[1].view(torch.int32)), f"{mode}: row scales differ"
    assert float(one[2].item()) == float(one[1].max().item()) > 0
