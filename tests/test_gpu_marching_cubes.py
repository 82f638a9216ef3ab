"""rnerf_marching_cubes_* / marching_cubes.marching_cubes on the device against the numpy oracle tests/helpers/marching_cubes_ref.py.

Parity is exact: faces integer-equal, vertices bit-equal as float64.  The oracle and the kernels apply the same individually rounded
float64 operations to the same float32 samples, and IEEE division has one answer, so a correct implementation has no freedom.

Timing: tools/marching_cubes_time.py (512^3 hull-like data, a smooth 257^3 field); DESIGN.md 3.10."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import marching_cubes_ref as MR             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = [(2, 2, 2), (3, 5, 67), (9, 6, 130), (17, 17, 17), (33, 20, 65)]        # no multiple of a brick; a cell either side of a 64-lane run


def run(field, iso):
    from samplenerfro_amd import marching_cubes
    v, f = marching_cubes.marching_cubes(field, iso, device=DEV)
    assert v.dtype == torch.float64 and f.dtype == torch.int32 and v.device == torch.device(DEV) and f.device == torch.device(DEV)
    assert v.ndim == 2 and v.shape[1] == 3 and f.ndim == 2 and f.shape[1] == 3
    return v.cpu().numpy(), f.cpu().numpy()


def assert_equals_oracle(field, iso):
    want_v, want_f = MR.marching_cubes(field, iso)
    v, f = run(field, iso)
    print(f"{tuple(np.shape(field))}: {len(want_v)} vertices, {len(want_f)} triangles")
    assert v.shape == want_v.shape and f.shape == want_f.shape
    assert np.array_equal(f, want_f)
    assert v.tobytes() == want_v.tobytes()                                   # bit-equal (and so NaN-free where the oracle is)
    return v, f


def smooth_field(dims, seed, waves=6, min_wavelength=5.0):
    """A sum of random plane waves, float32."""
    rng = np.random.default_rng(seed)
    x = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"), -1)
    out = np.zeros(dims)
    for _ in range(waves):
        k = rng.standard_normal(3)
        k *= 2 * np.pi / (min_wavelength * rng.uniform(1.0, 3.0) * np.linalg.norm(k))
        out += rng.uniform(0.5, 1.0) * np.sin(x @ k + rng.uniform(0, 2 * np.pi))
    return out.astype(np.float32)


def test_all_256_cases_stacked_along_z():
    """Every case once, as a zero-padded 4^3 block; the 1024 z samples of a row cross chunk and brick borders."""
    field = np.zeros((4, 4, 1024), np.float32)
    for case in range(256):
        for m in range(8):
            if (case >> m) & 1:
                field[1 + (m & 1), 1 + ((m >> 1) & 1), 4 * case + 1 + (m >> 2)] = 1.0
    v, f = assert_equals_oracle(field, 0.5)
    assert MR.is_closed_oriented(f) and len(v) == MR.num_crossed_edges(field, 0.5)
    assert np.all(np.isin(v * 2, np.arange(0, 2048)))                        # binary data: every vertex half way or on a node


@pytest.mark.parametrize("dims", DIMS)
def test_random_smooth_and_binary_fields(dims):
    assert_equals_oracle(smooth_field(dims, seed=sum(dims), min_wavelength=3.0), 0.1)
    rng = np.random.default_rng(100 + sum(dims))
    assert_equals_oracle(rng.random(dims) > 0.5, 0.5)                        # bool
    assert_equals_oracle((rng.random(dims) > 0.7).astype(np.uint8), 0.5)
    assert_equals_oracle(rng.standard_normal(dims), -0.3)                    # float64 noise: rounded to float32 first


def test_all_empty_and_all_solid_fields():
    for value in (0.0, 1.0):
        for dims in ((2, 2, 2), (9, 6, 130)):
            v, f = run(np.full(dims, value, np.float32), 0.5)
            torch.cuda.synchronize()
            assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = run(np.full((5, 5, 5), 0.5, np.float32), 0.5)                      # a plateau equal to iso has no surface inside it
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_ties_nan_and_infinities():
    dims, iso = (12, 11, 70), 0.25
    rng = np.random.default_rng(9)
    field = rng.uniform(-1, 1, dims).astype(np.float32)
    special = rng.random(dims)
    field[special < 0.10] = np.float32(iso)                                  # exact ties: empty, t = 0 against a solid neighbour
    field[(special >= 0.10) & (special < 0.15)] = np.nan                     # empty
    field[(special >= 0.15) & (special < 0.20)] = np.inf                     # solid
    field[(special >= 0.20) & (special < 0.25)] = -np.inf                    # empty
    field[6:9, 5:8, 30:40] = np.float32(iso)                                 # and a plateau of ties
    v, f = assert_equals_oracle(field, iso)
    assert np.all(np.isfinite(v)) and len(v) == MR.num_crossed_edges(field, iso)
    frac = v - np.floor(v)
    assert np.all((frac != 0).sum(1) <= 1)                                   # on its edge
    assert (frac == 0.5).any() and (frac.sum(1) == 0).any()                  # the t = 0.5 rule and t = 0 (tie or infinite neighbour) both occur
    assert v.min() >= 0 and np.all(v.max(0) <= np.array(dims) - 1)


def test_torus_is_closed_with_euler_characteristic_0():
    x, y, z = np.meshgrid(np.arange(65.0), np.arange(65.0), np.arange(33.0), indexing="ij")
    field = 8.0 - np.sqrt((np.sqrt((x - 32) ** 2 + (y - 32) ** 2) - 20.0) ** 2 + (z - 16) ** 2)
    v, f = assert_equals_oracle(field.astype(np.float32), 0.0)
    assert MR.is_closed_oriented(f) and MR.euler(v, f) == 0
    vol = MR.signed_volume(v, f)
    assert abs(vol / (2 * np.pi ** 2 * 20.0 * 64.0) - 1) < 0.02              # solid = the higher values: positive, 2 pi^2 R r^2


def test_more_bricks_than_one_pass_of_the_scan():
    """132 x 256 x 256 nodes are 8448 bricks of 1024; the scan takes 8192 per pass, so the last 256 bricks' offsets carry the first pass's
    totals.  Mostly empty, with a ball in the first pass's bricks and a box and single voxels in the second's: exact against the oracle."""
    field = np.zeros((132, 256, 256), np.float32)
    x, y, z = np.meshgrid(np.arange(40.0), np.arange(40.0), np.arange(40.0), indexing="ij")
    field[10:50, 100:140, 60:100] = 12.5 - np.sqrt((x - 19.3) ** 2 + (y - 20.1) ** 2 + (z - 19.6) ** 2)
    field[128:131, 250:255, 3:200] = 1.0
    field[129, 10, 10] = 0.5; field[130, 255, 254] = 2.0; field[131, 255, 255] = 3.0      # the very last node too
    assert field.size // 1024 > 8192 and field[:128].any() and field[128:].any()
    v, f = assert_equals_oracle(field, 0.25)
    assert len(v) == MR.num_crossed_edges(field, 0.25) and f.max() == len(v) - 1


@pytest.fixture(scope="module")
def big():
    """160^3, smooth (wavelengths of 16 samples and more) and empty on the boundary, so the surface stays inside the grid: five waves of
    amplitude below 1 against a radial ramp from +8 inside radius 60 to -8 beyond 80 (the faces' centres are at 79.5: below -7.6 + 5)."""
    G = 160
    r = np.linalg.norm(np.stack(np.meshgrid(*[np.arange(G) - (G - 1) / 2] * 3, indexing="ij"), -1), axis=-1)
    field = (smooth_field((G, G, G), seed=160, waves=5, min_wavelength=16.0) + 8.0 * np.clip((70.0 - r) / 10.0, -1.0, 1.0)).astype(np.float32)
    assert max(field[0].max(), field[-1].max(), field[:, 0].max(), field[:, -1].max(), field[:, :, 0].max(), field[:, :, -1].max()) < 0
    field.setflags(write=False)
    return field, torch.from_numpy(field.copy()).to(DEV)


def test_properties_at_160_cubed(big):
    from samplenerfro_amd import marching_cubes
    field, field_d = big
    v, f = marching_cubes.marching_cubes(field_d, 0.0)
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    print(f"160^3: {len(vn)} vertices, {len(fn)} triangles")
    assert len(vn) > 50000 and len(vn) == MR.num_crossed_edges(field, 0.0)
    assert MR.is_closed_oriented(fn) and fn.min() == 0 and fn.max() == len(vn) - 1
    assert (vn == np.round(vn)).sum(1).min() >= 2 and len(np.unique(vn, axis=0)) == len(vn)
    assert MR.signed_volume(vn, fn) > 0
    v2, f2 = marching_cubes.marching_cubes(field_d, 0.0)                     # two runs byte-identical
    assert torch.equal(v2, v) and torch.equal(f2, f)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # and the same on a non-default stream
        v3, f3 = marching_cubes.marching_cubes(field_d, 0.0)
    s.synchronize()
    assert torch.equal(v3, v) and torch.equal(f3, f)


def test_capacities_one_short_set_overflow_and_leave_the_guard_rows():
    from samplenerfro_amd import _lib
    lib = _lib.load()
    field = smooth_field((33, 20, 65), seed=7, min_wavelength=4.0)
    want_v, want_f = MR.marching_cubes(field, 0.1)
    V, F = len(want_v), len(want_f)
    assert V > 1000 and F > 1000
    f_d = torch.from_numpy(field).to(DEV)
    dims = (ctypes.c_int32 * 3)(*field.shape)
    ws = torch.empty(lib.rnerf_marching_cubes_workspace_bytes(ctypes.byref(dims)) // 8 + 1, dtype=torch.int64, device=DEV)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = _lib.current_stream()
    _lib.check(lib.rnerf_marching_cubes_count(_lib.ptr(f_d), ctypes.byref(dims), 0.1, _lib.ptr(ws), _lib.ptr(totals), st), "count")
    assert totals.tolist() == [V, F]
    GUARD = 4
    for cap_v, cap_f, want_overflow in ((V, F, 0), (V - 1, F, 1), (V, F - 1, 1), (V - 1, F - 1, 1), (V, 0, 0), (0, 0, 0), (0, F, 0)):     # the last: triangles alone, after a vertex launch
        verts = torch.full((V + GUARD, 3), -7.0, dtype=torch.float64, device=DEV)
        faces = torch.full((F + GUARD, 3), -7, dtype=torch.int32, device=DEV)
        overflow = torch.full((1,), 5, dtype=torch.int32, device=DEV)
        _lib.check(lib.rnerf_marching_cubes_emit(_lib.ptr(f_d), ctypes.byref(dims), 0.1, _lib.ptr(ws), _lib.ptr(verts), cap_v, _lib.ptr(faces), cap_f,
                                                 _lib.ptr(overflow), st), "emit")
        assert int(overflow.item()) == want_overflow, (cap_v, cap_f)
        vn, fn = verts.cpu().numpy(), faces.cpu().numpy()
        assert vn[:cap_v].tobytes() == want_v[:cap_v].tobytes() and np.all(vn[cap_v:] == -7.0), (cap_v, cap_f)
        assert np.array_equal(fn[:cap_f], want_f[:cap_f]) and np.all(fn[cap_f:] == -7), (cap_v, cap_f)


def test_voxelize_preview_mesh_on_the_example_grid(tmp_path):
    import cases
    from samplenerfro_amd import voxelize
    _, _, counts = cases.load_example_obj()
    data = cases.R.counts_to_ior(counts.astype(np.int32), 4).reshape(128, 128, 128)
    want_v, want_f = MR.marching_cubes(data, 1.165)
    v, f = voxelize.preview_mesh(torch.from_numpy(data).to(DEV), threshold=1.165, num_samples=4, extent=1.5, out_dir=str(tmp_path))
    assert np.array_equal(f.cpu().numpy(), want_f) and v.cpu().numpy().tobytes() == (want_v / 128 - 0.5).tobytes()
    v2, f2 = voxelize.load_obj(str(tmp_path / "mesh_4_128_1.5_1.165.obj"))     # the reference's file name; the bits survive the file
    assert v2.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(f2, want_f)
    vw, fw = voxelize.preview_mesh_world(data.reshape(-1, 1), threshold=1.165, extent=1.5, device=DEV)      # mesh.pkl's [G^3, 1] too
    assert np.array_equal(fw.cpu().numpy(), want_f) and vw.cpu().numpy().tobytes() == (want_v / 127.0 * 3.0 + -1.5).tobytes()


def test_visual_hull_preview_mesh_on_case_a():
    import make_visual_hull_reference as M
    from samplenerfro_amd import marching_cubes, visual_hull
    fx = np.load(M.OUT)
    count, V, G = fx["A_count"], len(fx["A_masks"]), int(fx["A_G"])
    lo, hi = fx["A_min_point"], fx["A_max_point"]
    inside = count.astype(np.float64) / V > 0.9
    assert np.array_equal((inside.reshape(-1, 1) * 0.33 + 1.0), fx["A_data"])  # the field is the hull the fixture's mesh.pkl holds
    want_v, want_f = MR.marching_cubes(inside, 0.5)
    assert len(want_f) > 100
    v, f = visual_hull.preview_mesh(torch.from_numpy(count).to(DEV), V, 0.9, lo, hi)
    assert np.array_equal(f.cpu().numpy(), want_f)
    assert v.cpu().numpy().tobytes() == (want_v / G * (hi - lo) + lo).tobytes()
    v2, _ = visual_hull.preview_mesh(count, V, 0.9, lo, hi, device=DEV)       # host counts are taken too
    assert torch.equal(v2, v)
    vi, fi = marching_cubes.marching_cubes(torch.from_numpy(inside).to(DEV), 0.5)
    vi = vi.cpu().numpy()
    assert np.array_equal(fi.cpu().numpy(), want_f)
    assert np.all((vi - np.floor(vi) == 0.5).sum(1) == 1) and np.all((vi == np.floor(vi)).sum(1) == 2)      # one half-integer coordinate


@pytest.fixture(scope="module")
def field_model():
    from samplenerfro_amd import models, synthetic as syn
    G = 8
    grid = syn.scale_ior(syn.sphere_grid(G, 1.5, 0.6), 0.5).astype(np.float32)
    model = models.NerfModel(ndim=[G] * 3, nmin=[-1.5] * 3, nmax=[1.5] * 3, grid=torch.from_numpy(grid).to(DEV), num_coarse_samples=16,
                             num_fine_samples=24, num_path_samples=4)
    pf = syn.init_params_flat(2, fine=True, bias_scale=0.05)
    variables = models.make_variables({k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in pf.items()})
    return model, variables


def test_alpha_grid_equals_sample_points(field_model):
    from samplenerfro_amd import extract
    model, variables = field_model
    t = np.linspace(-1.2, 1.2, 9).astype(np.float32)
    pts = torch.from_numpy(np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 1, 3)).to(DEV)
    assert pts.shape[0] == 729
    want = model.apply(variables, pts, torch.zeros_like(pts), method=model.sample_points)[1].reshape(9, 9, 9)
    for chunk in (1 << 18, 300):
        got = extract.alpha_grid(model, variables, resolution=8, range=1.2, chunk=chunk, device=DEV)
        assert got.dtype == torch.float32 and got.shape == (9, 9, 9) and got.device == torch.device(DEV)
        assert torch.equal(got, want), chunk


def test_extract_mesh_is_the_alpha_grids_surface_in_world_units(field_model):
    from samplenerfro_amd import extract
    model, variables = field_model
    alpha = extract.alpha_grid(model, variables, resolution=8, range=1.2, device=DEV)
    thr = float(alpha.median())
    want_v, want_f = MR.marching_cubes(alpha.cpu().numpy(), thr)
    assert len(want_f) > 0
    v, f = extract.extract_mesh(model, variables, resolution=8, range=1.2, threshold=thr, device=DEV)
    vn = v.cpu().numpy()
    assert np.array_equal(f.cpu().numpy(), want_f) and vn.tobytes() == (want_v / 8 * 2.4 - 1.2).tobytes()
    assert vn.min() >= -1.2 and vn.max() <= 1.2
