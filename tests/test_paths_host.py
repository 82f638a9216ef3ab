"""Host side of the bent-path diagnostics (no GPU): the line rule of tests/helpers/paths_ref.py held to its stated properties, the view
matrices, the ray colours and the pickle of samplenerfro_amd.paths against plt_utils.plot_path / extract_mesh.py, the argument checks,
and the summary restatement on the CPU oracle's march of a uniform grid and of a ball."""
import ctypes
import math
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import paths_ref as R               # noqa: E402

F32 = np.float32
SPAN = range(-9, 10)


def test_the_line_rule_hits_both_ends_is_connected_close_and_symmetric():
    for dx in SPAN:
        for dy in SPAN:
            x0, y0 = 3, -2
            px = R.line_pixels(x0, y0, x0 + dx, y0 + dy)
            n = max(abs(dx), abs(dy))
            assert len(px) == n + 1
            assert px[0] == (x0, y0) and px[-1] == (x0 + dx, y0 + dy)
            for (ax, ay), (bx, by) in zip(px, px[1:]):
                assert max(abs(bx - ax), abs(by - ay)) == 1                      # 8-connected, no pixel twice
            for i, (x, y) in enumerate(px):                                      # within half a pixel of the true line, exactly (integers)
                assert abs(2 * n * (x - x0) - 2 * i * dx) <= n and abs(2 * n * (y - y0) - 2 * i * dy) <= n
            assert set(px) == set(R.line_pixels(x0 + dx, y0 + dy, x0, y0))       # the same pixels in either direction


def test_the_clipped_walk_gives_the_pixels_inside_the_panel_and_is_short():
    size = 7
    for x0, y0 in ((-4, 2), (3, 3), (9, -1), (0, 6)):
        for dx in SPAN:
            for dy in SPAN:
                want = [(x, y) for x, y in R.line_pixels(x0, y0, x0 + dx, y0 + dy) if 0 <= x < size and 0 <= y < size]
                assert R.line_pixels_in_panel(x0, y0, x0 + dx, y0 + dy, size) == want
    far = 2 ** 30 - 1
    px = R.line_pixels_in_panel(-far, -far, far, far, size)                      # a diagonal of 2^31 pixels: `size` iterations
    assert px == [(i, i) for i in range(size)]
    # one row up over 2^31 - 2 columns: the step to row 4 is at the middle, column 0 (i = far: (2 far + 2 far) // (4 far) = 1)
    assert R.line_pixels_in_panel(-far, 3, far, 4, size) == [(x, 4) for x in range(size)]
    assert R.line_pixels_in_panel(-far, 3, far, 4 + far, size) == []             # leaves the panel's rows long before its columns


def test_view_matrices_are_orthonormal_up_to_scale_and_hold_the_cube():
    from samplenerfro_amd import paths
    center, side, size = np.array([0.3, -0.2, 1.1]), 2.5, 64
    m = paths.view_matrices(center, side, size)
    assert m.shape == (4, 2, 4) and m.dtype == np.float64
    scale = (size - 1) / (math.sqrt(3.0) * side)
    for (name, elev, azim), v in zip(paths.VIEWS, m):
        a, b = v[0, :3], v[1, :3]
        assert abs(a @ a - scale ** 2) < 1e-9 and abs(b @ b - scale ** 2) < 1e-9 and abs(a @ b) < 1e-9, name
        e, az = math.radians(elev), math.radians(azim)
        f = np.array([math.cos(e) * math.cos(az), math.cos(e) * math.sin(az), math.sin(e)])
        assert abs(a @ f) < 1e-9 and abs(b @ f) < 1e-9, name                     # both rows lie across the view direction
        assert np.allclose(v[:, :3] @ center + v[:, 3], size / 2)                # the centre lands in the middle
        for corner in np.ndindex(2, 2, 2):
            p = center + (np.array(corner) - 0.5) * side
            assert R.pixel(v, p) is not None
            x, y = R.pixel(v, p)
            assert 0 <= x < size and 0 <= y < size, (name, corner)
    assert [n for n, _, _ in paths.VIEWS] == ["top", "right", "front", "free"]
    assert [(e, a) for _, e, a in paths.VIEWS] == [(90, 0), (0, 0), (0, 90), (30, -60)]


def test_ray_colours_are_those_of_plot_path():
    from samplenerfro_amd import paths
    for n in (1, 2, 5, 9, 10, 256):
        sz = int(math.ceil(np.sqrt(n)))                                          # plot_path:38-40
        u, v = np.meshgrid(np.arange(sz + 1)[1:], np.arange(sz + 1)[1:], indexing="xy")
        color = np.stack([u, v, np.zeros_like(u)], axis=-1).reshape(-1, 3) / sz
        got = paths.ray_colours(n)
        assert got.dtype == np.uint8 and got.shape == (n, 3)
        assert np.array_equal(got, (color[:n] * 255).astype(np.uint8))
    assert paths.ray_colours(1).tolist() == [[255, 255, 0]]
    with pytest.raises(ValueError):
        paths.ray_colours(0)


def test_the_pickle_has_the_references_keys_shapes_and_name(tmp_path):
    from samplenerfro_amd import paths
    N, Nc = 24, 6
    rng = np.random.default_rng(0)
    rec = {"ray_pos": rng.standard_normal((1, N, 3)).astype(F32), "ray_dir": rng.standard_normal((1, N, 3)).astype(F32),
           "idx_grad": rng.standard_normal((1, N, 3)).astype(F32), "transform": np.eye(4, dtype=F32)[:3],
           "ray_pos_c": rng.standard_normal((1, Nc, 3)).astype(F32)}
    p = paths.save_ray_pkl(str(tmp_path), 0, 210, 244, rec)
    assert os.path.basename(p) == "ray_000_210_244.pkl" and os.listdir(tmp_path) == ["ray_000_210_244.pkl"]      # extract_mesh.py:216
    with open(p, "rb") as f:
        got = pickle.load(f)
    assert list(got) == ["ray_pos", "ray_dir", "idx_grad", "transform", "ray_pos_c"]                               # :217-223, in that order
    for k in got:
        assert np.array_equal(got[k], rec[k]) and got[k].dtype == F32
    assert got["ray_pos"].shape == (1, N, 3) and got["ray_pos_c"].shape == (1, Nc, 3)


def test_bad_indices_and_sizes_raise_on_the_host():
    torch = pytest.importorskip("torch")
    from samplenerfro_amd import paths
    pd = torch.zeros((5, 7, 4))                                                  # a CPU tensor: every check comes before the first launch
    for rays in ([7], [-1], [0, 3, 9], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            paths.plot_paths(pd, None, rays, size=16)
    for size in (7, 0, -3):
        with pytest.raises(ValueError):
            paths.plot_paths(pd, None, [0], size=size)
    with pytest.raises(ValueError):
        paths.plot_paths(pd, None, [0], size=16, frame="cube")
    with pytest.raises(ValueError):
        paths.plot_paths(pd, None, [0], size=16, frame="grid")                   # no box
    with pytest.raises(ValueError):
        paths.plot_paths(torch.zeros((5, 7, 3)), None, [0], size=16)
    with pytest.raises(ValueError):
        paths._pixel_indices([(4, 0)], 4, 6)
    with pytest.raises(ValueError):
        paths._pixel_indices([(0, -1)], 4, 6)
    assert paths._pixel_indices([(3, 5)], 4, 6).tolist() == [[3, 5]]


def test_argument_errors_of_the_entry_points_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p16 = ctypes.c_void_p(4096)
    assert lib.rnerf_path_summary(None, p16, p16, 4, 4, 1e-3, p16, p16, None) == -1 and b"rnerf_path_summary" in lib.rnerf_last_error()
    assert lib.rnerf_path_summary(p16, p16, p16, 0, 4, 1e-3, p16, p16, None) == -1
    assert lib.rnerf_path_summary(p16, p16, p16, 4, 0, 1e-3, p16, p16, None) == -1
    assert lib.rnerf_path_summary(p16, p16, ctypes.c_void_p(4100), 4, 4, 1e-3, p16, p16, None) == -1 and b"aligned" in lib.rnerf_last_error()
    assert lib.rnerf_path_summary(p16, p16, p16, 4, 4, float("nan"), p16, p16, None) == -1
    assert lib.rnerf_path_plot_workspace_bytes(4, 37) == (4 * 37 * 37 * 4 + 15) // 16 * 16
    assert lib.rnerf_path_plot_workspace_bytes(0, 37) == 0 and b"panels" in lib.rnerf_last_error()
    assert lib.rnerf_path_plot_workspace_bytes(9, 37) == 0 and lib.rnerf_path_plot_workspace_bytes(4, 0) == 0
    pan = (ctypes.c_double * 8)(*([0.0] * 8))
    assert lib.rnerf_path_plot(p16, None, 4, 4, p16, p16, 1, None, 1, 16, None, 0.0, 1e-3, p16, p16, None) == -1
    assert lib.rnerf_path_plot(p16, None, 4, 4, p16, p16, -1, pan, 1, 16, None, 0.0, 1e-3, p16, p16, None) == -1
    assert lib.rnerf_path_plot(None, None, 4, 4, p16, p16, 1, pan, 1, 16, None, 0.0, 1e-3, p16, p16, None) == -1
    assert lib.rnerf_path_plot(p16, None, 0, 4, p16, p16, 1, pan, 1, 16, None, 0.0, 1e-3, p16, p16, None) == -1
    assert lib.rnerf_path_plot(p16, None, 4, 4, p16, p16, 1, pan, 9, 16, None, 0.0, 1e-3, p16, p16, None) == -1
    assert b"rnerf_path_plot" in lib.rnerf_last_error()


# ---- the summary restatement on the CPU oracle's march -------------------------------------------------------------------------------
G, EXT, N = 12, 1.5, 24


def _march(grid, origins, viewdirs):
    from oracle import ref_np as O
    ndim, nmin, nmax = [G] * 3, [-EXT] * 3, [EXT] * 3
    table = O.build_table(grid, ndim, nmin, nmax)
    pos, dirs, dist, n, grad = O.path_sampler(origins, viewdirs, table, ndim, nmin, nmax, 2.0, 6.0, N)
    pd = np.concatenate([pos, dist[..., None]], -1).transpose(1, 0, 2)
    dr = np.concatenate([dirs, np.zeros_like(dist)[..., None]], -1).transpose(1, 0, 2)
    ior = np.concatenate([n, grad], -1).transpose(1, 0, 2)
    return np.ascontiguousarray(pd, F32), np.ascontiguousarray(dr, F32), np.ascontiguousarray(ior, F32)


def _rays():
    o = np.array([[-4.0, 0.02, 0.03], [-4.0, 1.4, 1.4], [0.05, -4.0, 0.0]], F32)          # through the centre, past the ball, through it along y
    d = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], F32)
    return o, d


def test_a_uniform_grid_bends_nothing():
    pd, dr, ior = _march(np.ones((G, G, G), F32), *_rays())
    nodes, maps = R.summary(pd, dr, ior)
    assert nodes.dtype == np.int32 and maps.dtype == F32 and nodes.shape == (3, 3) and maps.shape == (2, 3)
    assert nodes[0].tolist() == [0, 0, 0] and nodes[1].tolist() == [-1, -1, -1] and nodes[2].tolist() == [-1, -1, -1]
    assert maps[0].tolist() == [0.0, 0.0, 0.0] and maps[1].tolist() == [0.0, 0.0, 0.0]


def test_a_ball_bends_the_rays_that_meet_it():
    from oracle import ref_np as O
    from samplenerfro_amd import synthetic as syn
    grid = O.conv3d_normal(syn.scale_ior(syn.sphere_grid(G, EXT, 0.7), 0.5).reshape(-1, 1), [G] * 3, 3, 1.0).reshape(G, G, G)
    pd, dr, ior = _march(grid, *_rays())
    nodes, maps = R.summary(pd, dr, ior)
    for r in (0, 2):                                                             # the rays through the ball
        assert nodes[0, r] > 0 and 0 <= nodes[1, r] < nodes[2, r] < N
        assert maps[1, r] > 0.0 and np.isfinite(maps[0, r])
        m = R.refracting(ior)[:, r]
        assert m[nodes[1, r]] and m[nodes[2, r]] and not m[:nodes[1, r]].any() and not m[nodes[2, r] + 1:].any()
        assert nodes[0, r] == m.sum()
    # the ray that misses it: no node counts (the smoothed grid is 1 outside the ball only to rounding, so optical is not exactly 0)
    assert nodes[:, 1].tolist() == [0, -1, -1] and maps[0, 1] == 0.0 and abs(maps[1, 1]) < 1e-5
    # the optical thickness is about (n - 1) x chord: n = 1.5 inside a ball of radius 0.7, blurred over a coarse grid
    assert 0.2 < maps[1, 0] < 0.5 * 1.4 * 1.5


def test_the_summary_restatement_by_hand():
    # two nodes, one ray: a gradient of exactly float32(1e-3) is not refracting; optical = (1.5 - 1) x 2
    t = F32(1e-3)
    pd = np.array([[[0, 0, 0, 2]], [[2, 0, 0, 4]]], F32)
    dr = np.array([[[1, 0, 0, 0]], [[0, 1, 0, 0]]], F32)
    ior = np.array([[[1.5, t, 0, 0]], [[1.0, np.nextafter(t, F32(1)), 0, 0]]], F32)
    nodes, maps = R.summary(pd, dr, ior)
    assert nodes[:, 0].tolist() == [1, 1, 1]
    assert maps[0, 0] == np.sqrt(F32(2.0)) and maps[1, 0] == F32(1.0)
    ior[1, 0, 1] = np.nan
    assert R.summary(pd, dr, ior)[0][:, 0].tolist() == [0, -1, -1]
