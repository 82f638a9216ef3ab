"""rnerf_march_sparse (csrc/march.hip, march_kernel<..., SPARSE>): the march whose recorder wave writes the record of node k only where
sample_nodes[k // P] == k.  At those nodes the record — position, normalised direction, travelled distance — is the dense march's, bit
for bit; every other record of the two buffers is left exactly as it was; without sample_nodes the entry point is rnerf_march.

Shapes: 37 rays (not a multiple of the 16 rays of a workgroup: three workgroups, the last with surplus quads that replay a ray);
(N, P, Nc) = (48, 4, 12) — whole chunks of 6 nodes —, (50, 5, 10) — a partial last chunk, groups that straddle chunks — and (36, 12, 3) —
the flagship's P."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 37
POISON = 0x7FC0A5A5          # a quiet NaN with a payload no kernel produces
SHAPES = [(48, 4, 12), (50, 5, 10), (36, 12, 3)]
TABLES = ["sphere", "uniform", "sphere_bricks"]


@pytest.fixture(scope="module")
def scenes():
    """table name -> (model, origins, viewdirs); the dense records are cached per (table, N) and never modified."""
    from oracle import ref_np as R
    from samplenerfro_amd import models, synthetic as syn
    G, ext = 16, 1.5
    ndim, nmin, nmax = [G] * 3, [-ext] * 3, [ext] * 3
    sphere = R.conv3d_normal(syn.scale_ior(syn.sphere_grid(G, ext, 0.6), 0.5).reshape(-1, 1), ndim, 3, 1.0).reshape(ndim).astype(np.float32)
    grids = {"sphere": (sphere, "reference"), "uniform": (np.ones(ndim, np.float32), "reference"), "sphere_bricks": (sphere, "bricks")}
    o, d = syn.sphere_rays(B, seed=4)
    o, d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    out = {}
    for name, (g, layout) in grids.items():
        m = models.NerfModel(ndim=ndim, nmin=nmin, nmax=nmax, grid=torch.from_numpy(g).to(DEV), num_coarse_samples=12, num_fine_samples=0,
                             num_path_samples=4, precision="f16x3", table_layout=layout)
        out[name] = (m, o, d)
    out["_dense"] = {}
    return out


def _dense(scenes, table, N):
    from samplenerfro_amd import ops
    key = (table, N)
    if key not in scenes["_dense"]:
        m, o, d = scenes[table]
        pd, dr, _, _ = ops.march(m.table, m.spec, o, d, m.near, m.far, N)
        scenes["_dense"][key] = (pd, dr)
    return scenes["_dense"][key]


def _jitter(kind, N, P, Nc):
    base = np.arange(0, N, P, dtype=np.int32)
    if kind == "first":
        return base
    if kind == "last":
        return base + np.int32(P - 1)
    j = base + np.random.default_rng(100 * N + P).integers(0, P, Nc).astype(np.int32)
    j[0], j[-1] = 0, N - 1                                   # the first and the last node of the path are among the sampled ones
    return j


def _bits(t):
    return t.view(torch.int32)


def test_the_sphere_bends_the_rays_and_the_uniform_table_does_not(scenes):
    """What the two tables are there for: directions change along the path in the sphere, and stay the ray's in vacuum."""
    _, dr_s = _dense(scenes, "sphere", 48)
    _, dr_u = _dense(scenes, "uniform", 48)
    assert float((dr_s[-1, :, :3] - dr_s[0, :, :3]).abs().max()) > 1e-3
    assert torch.equal(dr_u[-1], dr_u[0])


@pytest.mark.parametrize("kind", ["first", "last", "random"])
@pytest.mark.parametrize("N,P,Nc", SHAPES)
@pytest.mark.parametrize("table", TABLES)
def test_sparse_march_writes_the_dense_bits_at_the_sampled_nodes_and_nothing_else(scenes, table, N, P, Nc, kind):
    from samplenerfro_amd import ops
    m, o, d = scenes[table]
    pd_ref, dr_ref = _dense(scenes, table, N)
    jit = _jitter(kind, N, P, Nc)
    assert jit.shape == (Nc,) and np.all(jit // P == np.arange(Nc))
    pd = torch.full((N, B, 4), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    dr = torch.full((N, B, 4), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    ops.march_sparse(m.table, m.spec, o, d, m.near, m.far, N, torch.from_numpy(jit).to(DEV), P, out=(pd, dr))
    torch.cuda.synchronize()
    sampled = torch.zeros(N, dtype=torch.bool, device=DEV)
    sampled[torch.from_numpy(jit).long().to(DEV)] = True
    for got, want in ((pd, pd_ref), (dr, dr_ref)):
        assert torch.equal(_bits(got)[sampled], _bits(want)[sampled])               # positions / directions and the distance (pd[..., 3])
        assert bool((_bits(got)[~sampled] == POISON).all())                           # not a byte of any other record
    assert bool(torch.isfinite(pd[sampled]).all()) and bool(torch.isfinite(dr[sampled]).all())


@pytest.mark.parametrize("N,P,Nc", SHAPES)
@pytest.mark.parametrize("table", TABLES)
def test_without_sample_nodes_the_entry_point_is_the_dense_march(scenes, table, N, P, Nc):
    from samplenerfro_amd import ops
    m, o, d = scenes[table]
    pd_ref, dr_ref = _dense(scenes, table, N)
    pd = torch.full((N, B, 4), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    dr = torch.full((N, B, 4), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    ops.march_sparse(m.table, m.spec, o, d, m.near, m.far, N, None, P, out=(pd, dr))
    assert torch.equal(_bits(pd), _bits(pd_ref)) and torch.equal(_bits(dr), _bits(dr_ref))


def test_argument_errors_are_status_codes(scenes):
    from samplenerfro_amd import _lib, ops
    m, o, d = scenes["sphere"]
    pd = torch.zeros((50, B, 4), device=DEV); dr = torch.zeros_like(pd)
    jit = torch.arange(0, 48, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.march_sparse(m.table, m.spec, o, d, m.near, m.far, 50, jit, 4, out=(pd, dr))       # 12 groups of 4 are not 50 nodes
    lib = _lib.load()
    import ctypes as C
    rc = lib.rnerf_march_sparse(m.table.data_ptr(), C.byref(m.spec), o.data_ptr(), d.data_ptr(), B, m.near, m.far, 50, pd.data_ptr(), dr.data_ptr(),
                                jit.data_ptr(), 4, _lib.current_stream())
    assert rc == -1 and b"multiple of num_path" in lib.rnerf_last_error()
