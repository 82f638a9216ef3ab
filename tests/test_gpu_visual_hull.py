"""rnerf_visual_hull_* / visual_hull.carve on the device against the counts the reference's own text computed
(tests/golden/visual_hull_reference.npz; cases A orbit, B default box with c <= 0 and a width of 72, C 70 views).

Every comparison is exact: counts are integers, and the fixture's inputs keep every in-window projection more than 1e-6 px from a
rounding boundary (tests/golden/make_visual_hull_reference.py) while float64 evaluation orders differ by about 1e-13 px.

Timing: tools/visual_hull_time.py (512^3 voxels x 100 views of 1080 x 1920); not yet run on an MI355X, no figure is claimed."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import make_visual_hull_reference as M      # noqa: E402
import visual_hull_ref                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx():
    return np.load(M.OUT)


def carve_case(fx, name, masks=None, **kw):
    from samplenerfro_amd import visual_hull
    x = M.load_case(fx, name)
    lo, hi = (None, None) if x["box"] is None else x["box"]
    return visual_hull.carve(x["masks"] if masks is None else masks, x["cam_mat"], x["transforms"], x["G"], min_point=lo, max_point=hi,
                             device=DEV, return_count=True, **kw)


@pytest.fixture(scope="module")
def carved(fx):
    """One carve of each case with the default chunking, shared by the tests below (never modified)."""
    return {name: carve_case(fx, name) for name in M.CASES}


@pytest.mark.parametrize("name", M.CASES)
def test_counts_and_grid_equal_the_references(fx, carved, name):
    data, ndim, nmin, nmax, count = carved[name]
    G = int(fx[f"{name}_G"])
    want = torch.from_numpy(fx[f"{name}_count"])
    got = count.cpu()
    print(f"{name}: {int((got != want).sum())} of {want.numel()} counts differ; hull {int((data > 1).sum())} voxels")
    assert count.dtype == torch.int32 and count.shape == (G, G, G) and torch.equal(got, want)
    assert data.dtype == torch.float32 and data.shape == (G, G, G) and data.device == torch.device(DEV)
    assert np.array_equal(data.cpu().numpy().reshape(-1, 1), fx[f"{name}_data"].astype(np.float32))
    assert ndim == [G] * 3 and nmin == [float(v) for v in fx[f"{name}_min_point"]] and nmax == [float(v) for v in fx[f"{name}_max_point"]]


def test_result_feeds_the_grid_preparation(fx, carved):
    """The tuple is voxelize.voxelize's: grid.prepare_grid / ops.grid_prefilter take it."""
    from samplenerfro_amd import grid
    data, ndim, nmin, nmax, _ = carved["A"]
    g = grid.prepare_grid(data.cpu().numpy().reshape(-1, 1), ndim, "glass", 3, 1.0, DEV)
    # a normalised blur of values in [1, 1.33] stays there up to float32 rounding of three 3-tap sums
    assert g.shape == tuple(ndim) and float(g.min()) >= 1.0 - 1e-5 and 1.0 < float(g.max()) <= 1.33 + 1e-5


@pytest.mark.parametrize("chunk", [1, 7, 64, 70])
def test_chunked_views_give_the_same_counts(fx, carved, chunk):
    data, *_, count = carve_case(fx, "C", views_per_chunk=chunk)
    assert torch.equal(count, carved["C"][4]) and torch.equal(data, carved["C"][0])


def test_a_second_run_is_bit_identical(fx, carved):
    for name in ("A", "B"):
        data, *_, count = carve_case(fx, name)
        assert torch.equal(count, carved[name][4]) and torch.equal(data, carved[name][0])


def test_from_calib_takes_the_references_dict(fx, carved):
    from samplenerfro_amd import visual_hull
    calib = {"cam_mat": fx["B_cam_mat"].tolist(), "frames": [{"file_path": f"{i}.jpg", "transform_matrix": t.tolist()} for i, t in enumerate(fx["B_transforms"])]}
    out = visual_hull.from_calib(calib, fx["B_masks"], 21, device=DEV, return_count=True)
    assert torch.equal(out[4], carved["B"][4]) and out[2] == carved["B"][2] and out[3] == carved["B"][3]


def test_accumulate_0_overwrites_and_1_adds(fx, carved):
    from samplenerfro_amd import _lib, visual_hull
    lib = _lib.load()
    x = M.load_case(fx, "A")
    G, (V, H, W) = x["G"], x["masks"].shape
    spec = _lib.Grid.make([G] * 3, x["box"][0], x["box"][1])
    m = torch.from_numpy(x["masks"]).to(DEV)
    pv = torch.from_numpy(visual_hull.projection_matrices(x["cam_mat"], x["transforms"])).to(DEV)
    ws = torch.empty(lib.rnerf_visual_hull_workspace_bytes(V, H, W) // 4, dtype=torch.int32, device=DEV)
    count = torch.full((G, G, G), -123456789, dtype=torch.int32, device=DEV)
    st = _lib.current_stream()
    call = lambda masks, acc: _lib.check(lib.rnerf_visual_hull_count(_lib.ptr(masks), V, H, W, _lib.ptr(pv), ctypes.byref(spec), acc,
                                                                     _lib.ptr(count), _lib.ptr(ws), st), "rnerf_visual_hull_count")
    call(m, 0)
    assert torch.equal(count, carved["A"][4])
    call(m, 1)
    assert torch.equal(count, 2 * carved["A"][4])
    call(None, 0)                                                            # masks == NULL: the workspace still holds these views' bits
    assert torch.equal(count, carved["A"][4])


def raw_counts(lib, masks, pv, G, lo, hi):
    """rnerf_visual_hull_count through the C ABI with the projection matrices given as they are."""
    from samplenerfro_amd import _lib
    V, H, W = masks.shape
    spec = _lib.Grid.make([G] * 3, lo, hi)
    m = torch.from_numpy(np.ascontiguousarray(masks)).to(DEV)
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(pv, np.float64).reshape(V, 12))).to(DEV)
    ws = torch.empty(lib.rnerf_visual_hull_workspace_bytes(V, H, W) // 4, dtype=torch.int32, device=DEV)
    count = torch.empty((G, G, G), dtype=torch.int32, device=DEV)
    rc = lib.rnerf_visual_hull_count(_lib.ptr(m), V, H, W, _lib.ptr(p), ctypes.byref(spec), 0, _lib.ptr(count), _lib.ptr(ws), _lib.current_stream())
    assert rc == 0, lib.rnerf_last_error()
    return count.cpu().numpy()


def boundary_case():
    """Projections that sit EXACTLY on rounding boundaries, where only the IEEE quotient and round-half-even give the reference's pixel.
    G = 9 on [-1, 1]: coordinates are multiples of 0.25, every product below is exact.
    View 0: c = 1, u = 2 x + 4.5, v = 2 y + 4.5 — integers and half-integers; a checkerboard mask makes the parity of the rounding count.
    View 1: c = z + 3, a = 2.5 c, b = 3.5 c — the quotients are 2.5 and 3.5 exactly although 1 / c is not representable: pixel
    (row 4, column 2) by round-half-even, the only pixel set."""
    pv = np.zeros((2, 3, 4))
    pv[0, 0, 0], pv[0, 0, 3], pv[0, 1, 1], pv[0, 1, 3], pv[0, 2, 3] = 2.0, 4.5, 2.0, 4.5, 1.0
    pv[1, 0, 2], pv[1, 0, 3], pv[1, 1, 2], pv[1, 1, 3], pv[1, 2, 2], pv[1, 2, 3] = 2.5, 7.5, 3.5, 10.5, 1.0, 3.0
    yy, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    masks = np.zeros((2, 8, 8), np.uint8)
    masks[0] = ((xx + yy) % 2) * 255
    masks[1, 4, 2] = 255
    return masks, pv


def test_projections_exactly_on_a_rounding_boundary():
    from samplenerfro_amd import _lib
    masks, pv = boundary_case()
    want = visual_hull_ref.counts_pv(masks, pv, 9, [-1.0] * 3, [1.0] * 3)
    assert np.all(want >= 1) and len(np.unique(want)) == 2                   # view 1 counts everywhere, view 0 on a checkerboard of voxels
    got = raw_counts(_lib.load(), masks, pv, 9, [-1.0] * 3, [1.0] * 3)
    assert np.array_equal(got, want)


def test_carve_on_the_current_device_when_none_is_named(fx, carved):
    from samplenerfro_amd import visual_hull
    x = M.load_case(fx, "C")
    data, ndim, nmin, nmax, count = visual_hull.carve(x["masks"], x["cam_mat"], x["transforms"], x["G"], min_point=x["box"][0],
                                                      max_point=x["box"][1], return_count=True)
    assert data.device == torch.device("cuda", torch.cuda.current_device()) and torch.equal(count, carved["C"][4])
    calib = {"cam_mat": x["cam_mat"].tolist(), "frames": [{"transform_matrix": t.tolist()} for t in x["transforms"]]}
    out = visual_hull.from_calib(calib, x["masks"], x["G"], min_point=x["box"][0], max_point=x["box"][1])
    assert len(out) == 4 and torch.equal(out[0], carved["C"][0])


def test_empty_and_full_masks(fx):
    x = M.load_case(fx, "B")
    V = len(x["masks"])
    data, *_, count = carve_case(fx, "B", masks=np.zeros_like(x["masks"]))
    assert int(count.abs().max()) == 0 and torch.all(data == 1.0)
    data, *_, count = carve_case(fx, "B", masks=np.full_like(x["masks"], 255))
    assert torch.all(count == V) and torch.all(data == np.float32(1.33))


def test_mask_containers_and_values_are_equivalent(fx, carved):
    m = fx["B_masks"]
    want = carved["B"][4]
    ones = (m > 0).astype(np.uint8)                                          # {0, 1}
    mixed = np.where((np.arange(m.size).reshape(m.shape) % 2) == 0, ones, m)  # {0, 1, 255}
    assert set(np.unique(mixed)) == {0, 1, 255}
    for masks in (m > 0, ones, mixed, torch.from_numpy(m), torch.from_numpy(m > 0), torch.from_numpy(m).to(DEV), list(m), [torch.from_numpy(a) for a in m]):
        assert torch.equal(carve_case(fx, "B", masks=masks)[4], want)


def test_a_nan_transform_clamps_into_the_image(fx):
    """c == 0 and NaN are unspecified in the reference; the device clamps to an in-range pixel.  One short call."""
    from samplenerfro_amd import visual_hull
    x = M.load_case(fx, "C")
    T = x["transforms"].copy()
    T[3, 1, 2] = np.nan
    T[5, :3, 3] = np.inf
    V = len(T)
    data, *_, count = visual_hull.carve(x["masks"], x["cam_mat"], T, x["G"], min_point=x["box"][0], max_point=x["box"][1], device=DEV,
                                        return_count=True)
    torch.cuda.synchronize()
    assert int(count.min()) >= 0 and int(count.max()) <= V
    assert bool(torch.all((data == 1.0) | (data == np.float32(1.33))))
    # the views that are finite still count as before: at most the two broken views differ
    assert int((count - np_to(fx["C_count"])).abs().max()) <= 2


def np_to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
