"""rnerf_components_* / components.py / the three consumers on the device against the numpy restatement of the canonical labels
(tests/helpers/components_ref.py).  Every comparison is exact: the outputs are integers (or values copied unchanged).

label() raises if a kernel set the iteration-cap error word, so every call below also checks that the word stayed zero.

Timing: tools/components_time.py (512^3)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import components_cases as cases            # noqa: E402
import components_ref as ref                # noqa: E402
import make_visual_hull_reference as M      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = cases.small_cases()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_labels(g, connectivity, phase, name):
    from samplenerfro_amd import components
    want = ref.label(g, connectivity, phase)
    s = dev(g)
    got = components.label(s, connectivity, phase)
    again = components.label(s, connectivity, phase)
    bad = int((got.cpu().numpy() != want).sum())
    print(f"{name} conn {connectivity} phase {phase}: {bad} of {want.size} labels differ, {len(np.unique(want[want >= 0]))} components")
    assert got.dtype == torch.int32 and tuple(got.shape) == g.shape and got.device == torch.device(DEV)
    assert bad == 0
    assert torch.equal(got, again)
    return got


@pytest.mark.parametrize("name", ["one_solid", "one_empty", "line_1x7x300", "cube_2x2x2"])
def test_labels_of_the_degenerate_shapes(name):
    for connectivity in (6, 18, 26):
        for phase in (1, 0):
            check_labels(CASES[name], connectivity, phase, name)


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("bernoulli")])
def test_labels_of_ragged_noise(name, connectivity):
    for phase in (1, 0):
        check_labels(CASES[name], connectivity, phase, name)


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("name", ["all_solid", "all_empty", "checkerboard", "snake", "corner_pairs", "edge_pairs"])
def test_labels_of_the_constructed_cases(name, connectivity):
    for phase in (1, 0):
        got = check_labels(CASES[name], connectivity, phase, name)
        k = int((got.reshape(-1) == torch.arange(got.numel(), device=DEV, dtype=torch.int32)).sum())
        if phase == 1:
            n = 11 ** 3
            expect = {"all_solid": [1, 1, 1], "all_empty": [0, 0, 0], "checkerboard": [365, 1, 1], "snake": [1, 1, 1],
                      "corner_pairs": [2 * n, 2 * n, n], "edge_pairs": [2 * n, n, n]}[name][(6, 18, 26).index(connectivity)]
            assert k == expect


def test_labels_of_160_cubed_noise():
    """1200 tiles; the giant component of p = 0.32 just above the percolation threshold runs through most of them."""
    check_labels(cases.bernoulli((160, 160, 160), 0.32, 160), 6, 1, "bernoulli_160")


def test_labels_next_to_the_index_limit():
    """1290^3 = 2 146 689 000 voxels, 794 647 below 2^31 - 1: every index form of the four kernels near its limit.  Closed-form input (the
    numpy helper would need tens of GB): a rod along x through every x-tile from voxel 0, a row along z in the last (x, y) column, and
    the very last voxel on its own."""
    from samplenerfro_amd import components
    G = 1290
    n = G ** 3
    assert 2 ** 31 - 1 - 10 ** 6 < n <= 2 ** 31 - 1
    solid = torch.zeros((G, G, G), dtype=torch.uint8, device=DEV)
    solid[:, 0, 0] = 1
    solid[-1, -1, :-2] = 1
    solid[-1, -1, -1] = 1
    labels = components.label(solid, 6)
    assert int((labels >= 0).sum()) == G + (G - 2) + 1
    assert bool((labels[:, 0, 0] == 0).all()) and bool((labels[-1, -1, :-2] == n - G).all()) and int(labels[-1, -1, -1]) == n - 1
    assert int(labels[-1, -1, -2]) == -1
    size, border, counts = components.raw_stats(labels)
    assert counts.tolist() == [3, 2 * G - 1]
    flat = size.reshape(-1)
    assert int(flat[0]) == G and int(flat[n - G]) == G - 2 and int(flat[n - 1]) == 1 and int(flat.sum(dtype=torch.int64)) == 2 * G - 1
    assert int(border.sum(dtype=torch.int64)) == 3
    keep = torch.zeros(n, dtype=torch.uint8, device=DEV); keep[0] = 1
    del size, border
    components.apply(solid, labels, keep, 0)
    assert int(solid.sum(dtype=torch.int64)) == G and bool((solid[:, 0, 0] == 1).all())
    # the empty phase of what is left: one component of n - G voxels whose smallest index is 1
    del labels, keep
    empty = components.label(solid, 26, 0)
    assert int((empty >= 0).sum(dtype=torch.int64)) == n - G and int(empty.max()) == 1 and int(empty[0, 0, 0]) == -1


def test_stats_equal_the_helpers():
    from samplenerfro_amd import components
    two = np.zeros((6, 6, 12), np.uint8); two[3:5, 3:5, 8:10] = 1; two[0:2, 0:2, 0:2] = 1
    for name, g, connectivity in [("noise", CASES["bernoulli_33x20x70_p0.32"], 6), ("noise26", CASES["bernoulli_17x9x130_p0.5"], 26),
                                  ("two_cubes", two, 6), ("all_solid", CASES["all_solid"], 6), ("all_empty", CASES["all_empty"], 18)]:
        want_labels = ref.label(g, connectivity)
        labels = components.label(dev(g), connectivity)
        size, border, counts = components.raw_stats(labels)
        flat = want_labels.reshape(-1)
        assert np.array_equal(size.cpu().numpy().reshape(-1), np.bincount(flat[flat >= 0], minlength=flat.size)), name
        roots, sizes, brd = components.stats(labels)
        wr, ws, wb = ref.stats(want_labels)
        assert roots.dtype == torch.int32 and sizes.dtype == torch.int64 and brd.dtype == torch.bool
        assert np.array_equal(roots.cpu().numpy(), wr) and np.array_equal(sizes.cpu().numpy(), ws) and np.array_equal(brd.cpu().numpy(), wb), name
        assert int(border.sum()) == int(wb.sum()) and counts.tolist() == [len(wr), int((flat >= 0).sum())], name
        size2, border2, counts2 = components.raw_stats(labels)
        assert torch.equal(size, size2) and torch.equal(border, border2) and torch.equal(counts, counts2)
    roots, sizes, _ = components.stats(components.label(dev(two)))
    assert roots.tolist() == [0, (3 * 6 + 3) * 12 + 8] and sizes.tolist() == [8, 8]          # equal sizes: the lower root first


def test_select_on_the_shell():
    from samplenerfro_amd import components
    g, shell, cavity = cases.shell_scene()
    mask, info = components.select(dev(g), keep=1)
    assert np.array_equal(mask.cpu().numpy() != 0, shell)
    assert (info["components"], info["kept"], info["dropped"], info["voxels_dropped"], info["voxels_filled"]) == (4, 1, 3, 24, 0)
    assert info["sizes"].tolist() == [int(shell.sum()), 8, 8, 8]
    mask, info = components.select(dev(g), keep=1, fill_holes=True)
    assert np.array_equal(mask.cpu().numpy() != 0, shell | cavity) and info["voxels_filled"] == int(cavity.sum())
    # min_voxels alone: everything of at least 8 voxels stays; 9 leaves the shell
    assert np.array_equal(components.select(dev(g), keep=None, min_voxels=8)[0].cpu().numpy(), g)
    assert np.array_equal(components.select(dev(g), keep=None, min_voxels=9)[0].cpu().numpy() != 0, shell)
    for kw in (dict(keep=2), dict(keep=3, connectivity=26), dict(keep=None, min_voxels=9, fill_holes=True, connectivity=18)):
        want = ref.select(g, **kw)[0]
        assert np.array_equal(components.select(dev(g), **kw)[0].cpu().numpy() != 0, want), kw


def test_tunnels_and_open_cavities_are_not_filled():
    from samplenerfro_amd import components
    t = cases.torus()
    mask, info = components.select(dev(t), keep=1, fill_holes=True)
    assert np.array_equal(mask.cpu().numpy(), t) and info["voxels_filled"] == 0 and info["components"] == 1
    mask, info = components.select(dev(cases.box_with_cavity(None)), fill_holes=True)
    assert info["voxels_filled"] == 27 and int(mask.sum()) == 9 ** 3
    for channel in ("straight", "diagonal"):
        g = cases.box_with_cavity(channel)
        mask, info = components.select(dev(g), connectivity=6, fill_holes=True)          # empty phase: 26
        assert info["voxels_filled"] == 0 and np.array_equal(mask.cpu().numpy(), g), channel
    g = cases.box_with_cavity("diagonal")
    mask, info = components.select(dev(g), connectivity=26, fill_holes=True)               # empty phase: 6, the diagonal steps are walls
    assert np.array_equal(mask.cpu().numpy() != 0, ref.select(g, connectivity=26, fill_holes=True)[0]) and info["voxels_filled"] == 29


def test_the_identity_arguments_return_the_input_bit_for_bit():
    from samplenerfro_amd import components
    g = CASES["bernoulli_33x20x70_p0.32"] * np.uint8(201)          # non-zero values other than 1 stay what they are
    s = dev(g)
    mask, info = components.select(s, keep=None, min_voxels=1, fill_holes=False)
    assert mask.dtype == torch.uint8 and torch.equal(mask, s) and mask.data_ptr() != s.data_ptr()
    assert info["dropped"] == 0 and info["voxels_dropped"] == 0 and info["voxels_filled"] == 0
    b = dev(g != 0)
    mask, _ = components.select(b, keep=None)
    assert mask.dtype == torch.bool and torch.equal(mask, b)


def test_apply_rewrites_the_three_payloads():
    from samplenerfro_amd import components
    g, shell, cavity = cases.shell_scene()
    s = dev(g)
    labels = components.label(s)
    roots, sizes, _ = components.stats(labels)
    keep = torch.zeros(g.size, dtype=torch.uint8, device=DEV); keep[roots[:1].long()] = 1
    gone = torch.from_numpy((g != 0) & ~shell).to(DEV)
    for dtype, drop in ((torch.uint8, 7), (torch.int32, -5), (torch.float32, 0.25)):
        payload = (torch.arange(g.size, device=DEV) % 200 + 20).reshape(g.shape).to(dtype)
        out = components.apply(payload.clone(), labels, keep, drop)
        assert torch.equal(out[gone], torch.full_like(out[gone], drop)) and torch.equal(out[~gone], payload[~gone])


# ---- the consumers -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx():
    return np.load(M.OUT)


def carve_case(fx, name, **kw):
    from samplenerfro_amd import visual_hull
    x = M.load_case(fx, name)
    lo, hi = (None, None) if x["box"] is None else x["box"]
    return visual_hull.carve(x["masks"], x["cam_mat"], x["transforms"], x["G"], min_point=lo, max_point=hi, device=DEV, return_count=True, **kw)


@pytest.fixture(scope="module")
def carved(fx):
    return {name: carve_case(fx, name) for name in M.CASES}


def want_clean(count, V, threshold, **kw):
    """(data, count_clean) of visual_hull.clean from the helper."""
    c = count.cpu().numpy()
    solid = c.astype(np.float64) / V > threshold
    mask, dropped, filled = ref.select(solid, **kw)
    cc = c.copy(); cc[dropped] = 0; cc[filled] = V
    return np.where(mask, np.float32(1.33), np.float32(1.0)), cc


@pytest.mark.parametrize("name", M.CASES)
def test_visual_hull_clean_on_the_fixtures(fx, carved, name):
    from samplenerfro_amd import visual_hull
    data, ndim, nmin, nmax, count = carved[name]
    V = int(fx[f"{name}_masks"].shape[0])
    d, cc, info = visual_hull.clean(count, V, M.THRESHOLD, keep=None, min_voxels=1, fill_holes=False)
    assert torch.equal(d, data) and torch.equal(cc, count) and cc.data_ptr() != count.data_ptr() and info["dropped"] == 0
    for kw in (dict(keep=1, fill_holes=False), dict(keep=1, fill_holes=True), dict(keep=None, min_voxels=3, connectivity=26, fill_holes=True)):
        d, cc, info = visual_hull.clean(count, V, M.THRESHOLD, **kw)
        wd, wc = want_clean(count, V, M.THRESHOLD, **kw)
        print(f"{name} {kw}: {info['components']} components, {info['voxels_dropped']} voxels dropped, {info['voxels_filled']} filled")
        assert d.dtype == torch.float32 and cc.dtype == torch.int32
        assert np.array_equal(d.cpu().numpy(), wd) and np.array_equal(cc.cpu().numpy(), wc), kw


def test_visual_hull_clean_removes_a_planted_floater(fx, carved, tmp_path):
    import pickle
    from samplenerfro_amd import visual_hull
    data, ndim, nmin, nmax, count = carved["A"]
    V, G = int(fx["A_masks"].shape[0]), int(fx["A_G"])
    d0, c0, info0 = visual_hull.clean(count, V, M.THRESHOLD, keep=1, fill_holes=False)
    planted = count.clone()
    assert int(planted[:3, :3, :3].max()) * 1.0 / V <= M.THRESHOLD          # the corner is empty, also next to the floater
    planted[:2, :2, :2] = V
    d1, c1, info1 = visual_hull.clean(planted, V, M.THRESHOLD, keep=1, fill_holes=False)
    assert info1["components"] == info0["components"] + 1 and info1["voxels_dropped"] == info0["voxels_dropped"] + 8
    assert int(c1[:2, :2, :2].abs().sum()) == 0 and torch.equal(d1, d0)
    rest = torch.ones_like(count, dtype=torch.bool); rest[:2, :2, :2] = False
    assert torch.equal(c1[rest], c0[rest])
    # save_mesh_pkl and preview_mesh on count_clean agree with data
    path = str(tmp_path / "mesh.pkl")
    visual_hull.save_mesh_pkl(path, c1, V, M.THRESHOLD, nmin, nmax)
    with open(path, "rb") as f:
        saved = pickle.load(f)["data"]
    assert np.array_equal(saved.astype(np.float32).reshape(G, G, G), d1.cpu().numpy())
    assert np.array_equal(saved, (d1.cpu().numpy().reshape(-1, 1) > 1.0) * 0.33 + 1.0)
    verts, faces = visual_hull.preview_mesh(c1, V, M.THRESHOLD, nmin, nmax)
    kept = torch.nonzero(d1 > 1.0).to(torch.float64)
    lo = visual_hull.preview_coords(kept.min(0).values - 1.0, G, nmin, nmax)
    hi = visual_hull.preview_coords(kept.max(0).values + 1.0, G, nmin, nmax)
    assert verts.shape[0] > 0 and bool((verts >= lo).all()) and bool((verts <= hi).all())
    # the floater did reach the mesh before the clean-up
    verts_p, _ = visual_hull.preview_mesh(planted, V, M.THRESHOLD, nmin, nmax)
    assert not (bool((verts_p >= lo).all()) and bool((verts_p <= hi).all()))


def test_carve_with_clean_equals_carve_then_clean(fx, carved):
    from samplenerfro_amd import visual_hull
    for name, kw in (("A", dict(keep=1)), ("B", dict(keep=1, min_voxels=2, connectivity=18, fill_holes=False))):
        data, ndim, nmin, nmax, count = carved[name]
        V = int(fx[f"{name}_masks"].shape[0])
        d, cc, _ = visual_hull.clean(count, V, M.THRESHOLD, **kw)
        got = carve_case(fx, name, clean=kw)
        assert torch.equal(got[0], d) and torch.equal(got[4], cc) and got[1:4] == (ndim, nmin, nmax)
        plain = carve_case(fx, name, clean=None)
        assert torch.equal(plain[0], data) and torch.equal(plain[4], count)


def test_voxelize_clean():
    from samplenerfro_amd import voxelize
    g, shell, cavity = cases.shell_scene()
    rng = np.random.default_rng(5)
    data = np.where(g != 0, 1.0 + 0.33 * rng.integers(1, 65, g.shape) / 64.0, 1.0).astype(np.float32)          # mean IoRs of 1 .. 64 of 64 sub-samples
    out, info = voxelize.clean(dev(data), keep=1)
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), np.where(shell, data, np.float32(1.0))) and info["voxels_dropped"] == 24
    out, info = voxelize.clean(dev(data), keep=1, fill_holes=True)
    want = np.where(shell, data, np.float32(1.0)); want[cavity] = np.float32(1.33)
    assert np.array_equal(out.cpu().numpy(), want) and info["voxels_filled"] == int(cavity.sum())
    out, info = voxelize.clean(dev(data), keep=None)
    assert np.array_equal(out.cpu().numpy(), data) and info["dropped"] == 0


def test_extract_mesh_keeps_the_largest_component(monkeypatch):
    from samplenerfro_amd import extract, marching_cubes
    N = 24
    alpha = np.full((N + 1,) * 3, 0.02, np.float32)
    alpha[cases.ball((N + 1,) * 3, (12, 12, 12), 6)] = 0.8
    alpha[3:5, 3:5, 19:21] = 0.6          # a floater above the threshold
    alpha[20, 20, 3] = 0.09               # and one below it
    calls = []
    monkeypatch.setattr(extract, "alpha_grid", lambda *a, **k: (calls.append(1), dev(alpha))[1])
    solid = alpha.astype(np.float64) > 0.1
    want_alpha = np.where(ref.select(solid, keep=1)[0] | ~solid, alpha, np.float32(0.0))
    wv, wf = marching_cubes.marching_cubes(dev(want_alpha), 0.1)
    verts, faces = extract.extract_mesh(None, None, resolution=N, range=1.2, threshold=0.1, keep=1)
    assert torch.equal(faces, wf) and torch.equal(verts, wv / torch.full((3,), float(N), dtype=torch.float64, device=DEV) * 2.4 - 1.2)
    v0, f0 = extract.extract_mesh(None, None, resolution=N, range=1.2, threshold=0.1)          # the defaults: the floater's crumbs are there
    pv, pf = marching_cubes.marching_cubes(dev(alpha), 0.1)
    assert torch.equal(f0, pf) and f0.shape[0] > faces.shape[0] and len(calls) == 2
