"""Visual-hull carving without a GPU.

- tests/helpers/visual_hull_ref.py (an independent numpy restatement, a loop over voxel rows) against
  tests/golden/visual_hull_reference.npz, which tests/golden/make_visual_hull_reference.py computed by running the reference's own
  to_view_matrix / project_2d / create_init_bounding_box (re-run here where the reference exists);
- the host half of samplenerfro_amd/visual_hull.py: view matrices, the default box, mesh.pkl;
- the C ABI: the new symbols are declared, bound and exported, and argument errors are reported without a device.

Every comparison is exact.  The fixture's inputs keep every in-window projection more than 1e-6 px from a rounding boundary (stored
minima, checked below) while two float64 evaluation orders differ by about 1e-13 px, so a correct implementation has no freedom."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_visual_hull_reference as M      # noqa: E402
import visual_hull_ref                      # noqa: E402

FIXTURE = M.OUT


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE)


def test_fixture_is_small_and_its_cases_are_what_they_claim(fx):
    assert os.path.getsize(FIXTURE) < 150 * 1024
    shapes = {"A": (24, 8, 48, 64), "B": (21, 6, 40, 72), "C": (12, 70, 16, 20)}
    for name, (G, V, H, W) in shapes.items():
        assert int(fx[f"{name}_G"]) == G and fx[f"{name}_masks"].shape == (V, H, W) and fx[f"{name}_masks"].dtype == np.uint8
        assert fx[f"{name}_transforms"].shape == (V, 4, 4) and fx[f"{name}_count"].shape == (G, G, G)
        assert fx[f"{name}_data"].shape == (G ** 3, 1) and fx[f"{name}_data"].dtype == np.float64
        # the conditions that make exact equality a fair demand, and a non-trivial answer
        assert float(fx[f"{name}_min_half_dist"]) > 1e-6 and float(fx[f"{name}_min_abs_c"]) > 1e-6
        assert float(fx[f"{name}_order_diff"]) < 1e-9
        hull = fx[f"{name}_data"] > 1.0
        assert 0 < hull.sum() < hull.size and len(np.unique(fx[f"{name}_count"])) >= 5
        assert fx[f"{name}_count"].min() >= 0 and fx[f"{name}_count"].max() <= V
    assert int(fx["A_num_clipped_inside"]) > 0 and not bool(fx["A_default_box"])
    assert int(fx["B_num_c_le_0"]) > 0 and bool(fx["B_default_box"])
    assert float(fx["threshold"]) == 0.9


@pytest.mark.parametrize("name", M.CASES)
def test_restatement_reproduces_the_references_counts(fx, name):
    x = M.load_case(fx, name)
    lo, hi = fx[f"{name}_min_point"], fx[f"{name}_max_point"]
    c = visual_hull_ref.counts(x["masks"], x["cam_mat"], x["transforms"], x["G"], lo, hi)
    assert np.array_equal(c, fx[f"{name}_count"])
    assert np.array_equal(visual_hull_ref.grid_values(c, len(x["masks"])), fx[f"{name}_data"])
    if x["box"] is None:
        blo, bhi = visual_hull_ref.default_box(x["transforms"])
        assert np.array_equal(blo, lo) and np.array_equal(bhi, hi)


def test_generator_reproduces_the_committed_file():
    if M.source_sha256() is None:
        pytest.skip("the reference checkout is not on this machine")
    assert M.check(FIXTURE)


def test_view_matrices_and_default_box_equal_the_references(fx):
    from samplenerfro_amd import visual_hull
    for name in M.CASES:
        T = fx[f"{name}_transforms"]
        for t, want in zip(T, fx[f"{name}_view_mats"]):
            assert np.array_equal(visual_hull.to_view_matrix(t), want)
        pv = visual_hull.projection_matrices(fx[f"{name}_cam_mat"], T)
        assert pv.shape == (len(T), 12) and pv.dtype == np.float64
        p_mat = np.concatenate([fx[f"{name}_cam_mat"], np.zeros((3, 1))], axis=1)
        assert np.array_equal(pv[0].reshape(3, 4), p_mat @ fx[f"{name}_view_mats"][0])
    lo, hi = visual_hull.init_bounding_box(fx["B_transforms"])              # (min, max): the reference returns (max, min)
    assert np.array_equal(lo, fx["B_min_point"]) and np.array_equal(hi, fx["B_max_point"]) and np.all(lo < hi)
    lo, hi = visual_hull.init_bounding_box(list(fx["B_transforms"]))
    assert np.array_equal(lo, fx["B_min_point"]) and np.array_equal(hi, fx["B_max_point"])


@pytest.mark.parametrize("name", M.CASES)
def test_mesh_pkl_round_trip_equals_the_references_array(fx, name, tmp_path):
    import pickle
    from samplenerfro_amd import grid, visual_hull
    G, V = int(fx[f"{name}_G"]), len(fx[f"{name}_masks"])
    lo, hi = fx[f"{name}_min_point"], fx[f"{name}_max_point"]
    path = str(tmp_path / "mesh.pkl")
    visual_hull.save_mesh_pkl(path, fx[f"{name}_count"], V, 0.9, lo, hi)
    with open(path, "rb") as f:
        d = pickle.load(f)
    assert sorted(d) == ["data", "extent", "max_point", "min_point", "num_voxels"]               # make_visual_hull.py:139-146
    assert d["extent"] == 0 and d["num_voxels"] == G
    assert d["data"].dtype == np.float64 and np.array_equal(d["data"], fx[f"{name}_data"])
    data, ndim, nmin, nmax = grid.load_mesh_pkl(path)
    assert np.array_equal(data, fx[f"{name}_data"]) and ndim == [G, G, G]
    assert nmin == [float(v) for v in lo] and nmax == [float(v) for v in hi]
    import torch
    visual_hull.save_mesh_pkl(path, torch.from_numpy(fx[f"{name}_count"]), V, 0.9, lo, hi)      # a tensor of counts is taken too
    assert np.array_equal(grid.load_mesh_pkl(path)[0], fx[f"{name}_data"])
    with pytest.raises(ValueError):
        visual_hull.save_mesh_pkl(path, fx[f"{name}_count"].reshape(-1), V, 0.9, lo, hi)


NEW_SYMBOLS = ("rnerf_visual_hull_workspace_bytes", "rnerf_visual_hull_pack", "rnerf_visual_hull_count", "rnerf_visual_hull_finalize")


def test_new_symbols_are_declared_bound_and_exported(lib_path):
    from samplenerfro_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rnerf.h")).read()
    lib = ctypes.CDLL(lib_path)
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.load().rnerf_version() == 4                                  # appended: the ABI version does not move
    import samplenerfro_amd
    assert samplenerfro_amd.visual_hull.carve is not None


def test_argument_errors_and_workspace_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    cube = _lib.Grid.make([8, 8, 8], [-1, -1, -1], [1, 1, 1])
    g = ctypes.byref(cube)
    err = lambda: lib.rnerf_last_error()

    # one bit per pixel, rows padded to 32-bit words
    assert lib.rnerf_visual_hull_workspace_bytes(100, 1080, 1920) == 100 * 1080 * 60 * 4
    assert lib.rnerf_visual_hull_workspace_bytes(6, 40, 72) == 6 * 40 * 3 * 4
    assert lib.rnerf_visual_hull_workspace_bytes(1, 1, 1) == 4
    for V, H, W in ((0, 40, 72), (-1, 40, 72), (1, 0, 72), (1, 40, 0), (1, 65536, 32768)):
        assert lib.rnerf_visual_hull_workspace_bytes(V, H, W) == 0 and b"num_views" in err()
        assert lib.rnerf_visual_hull_count(p, V, H, W, p, g, 0, p, p, None) == -1 and b"num_views" in err()
        assert lib.rnerf_visual_hull_pack(p, V, H, W, p, None) == -1

    # null pointers
    assert lib.rnerf_visual_hull_count(p, 2, 40, 72, None, g, 0, p, p, None) == -1 and b"null pointer" in err()
    assert lib.rnerf_visual_hull_count(p, 2, 40, 72, p, None, 0, p, p, None) == -1 and b"null pointer" in err()
    assert lib.rnerf_visual_hull_count(p, 2, 40, 72, p, g, 0, None, p, None) == -1
    assert lib.rnerf_visual_hull_count(p, 2, 40, 72, p, g, 0, p, None, None) == -1
    assert lib.rnerf_visual_hull_pack(None, 2, 40, 72, p, None) == -1 and b"null pointer" in err()
    assert lib.rnerf_visual_hull_finalize(None, g, 2, 0.9, 1.33, 1.0, p, None) == -1 and b"null pointer" in err()
    assert lib.rnerf_visual_hull_finalize(p, g, 2, 0.9, 1.33, 1.0, None, None) == -1

    # grids: cubic only, 2 <= G, G^3 < 2^31
    for dims in ([8, 8, 9], [9, 8, 8], [1, 1, 1], [1291, 1291, 1291]):
        bad = _lib.Grid.make(dims, [-1, -1, -1], [1, 1, 1])
        assert lib.rnerf_visual_hull_count(p, 2, 40, 72, p, ctypes.byref(bad), 0, p, p, None) == -1 and b"cubic" in err()
        assert lib.rnerf_visual_hull_finalize(p, ctypes.byref(bad), 2, 0.9, 1.33, 1.0, p, None) == -1 and b"cubic" in err()

    assert lib.rnerf_visual_hull_count(p, 2, 40, 72, p, g, 2, p, p, None) == -1 and b"accumulate" in err()
    assert lib.rnerf_visual_hull_count(p, 2, 40, 72, p, g, 0, p, ctypes.c_void_p(258), None) == -1 and b"aligned" in err()
    assert lib.rnerf_visual_hull_finalize(p, g, 0, 0.9, 1.33, 1.0, p, None) == -1 and b"total_views" in err()


def test_carve_rejects_bad_inputs_before_any_device_work(fx):
    from samplenerfro_amd import visual_hull
    x = M.load_case(fx, "B")
    with pytest.raises(ValueError):
        visual_hull.carve(x["masks"], x["cam_mat"], x["transforms"][:-1], 8)                      # one transform short
    with pytest.raises(ValueError):
        visual_hull.carve(x["masks"].astype(np.float32), x["cam_mat"], x["transforms"], 8)
    with pytest.raises(ValueError):
        visual_hull.carve(x["masks"][0], x["cam_mat"], x["transforms"], 8)                        # [H, W]
    with pytest.raises(ValueError):
        visual_hull.carve([x["masks"][0], x["masks"][1][:, :-1]], x["cam_mat"], x["transforms"][:2], 8)     # per-view sizes differ
    import torch
    with pytest.raises(ValueError):                                                               # the same for a list of tensors
        visual_hull.carve([torch.from_numpy(x["masks"][0]), torch.from_numpy(x["masks"][1][:, :-1].copy())], x["cam_mat"], x["transforms"][:2], 8)
    with pytest.raises(ValueError):
        visual_hull.carve(x["masks"], np.eye(4), x["transforms"], 8)
