"""Host side of the synthetic-scene renderer (no GPU): the two entry points are declared, exported and bound and refuse bad arguments
before any device work; the cameras of samplenerfro_amd.scenes; the procedural environment; and the cube-map convention of
tests/helpers/scene_ref.py (the restatement the device's shading is held to) on the directions where the face choice is a tie."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import scene_ref as R               # noqa: E402

F32 = np.float32


def test_symbols_are_declared_exported_and_bound(lib_path):
    from samplenerfro_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "rnerf.h")).read()
    lib = ctypes.CDLL(lib_path)
    for name in ("rnerf_scene_trace", "rnerf_scene_shade"):
        assert f"int {name}(" in hdr and hasattr(lib, name) and name in _lib.SIGNATURES
    assert "scene.hip" in build.SOURCES
    assert _lib.load().rnerf_version() == 4


def test_argument_errors_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p
    T, O, V, X, C, ENV, RGB, TR, M = (0x100000 * k for k in range(1, 10))      # never dereferenced: every call fails first
    g = _lib.Grid.make([8, 8, 8], [-1] * 3, [1] * 3)
    nan = float("nan")

    def trace(t=T, grid=g, o=O, v=V, B=4, N=8, n_in=1.2, eps=1e-3, x=X, c=C):
        return lib.rnerf_scene_trace(p(t), ctypes.byref(grid) if grid is not None else None, p(o), p(v), B, 2.0, 6.0, N, n_in, eps, p(x), p(c), None)

    for bad in (dict(t=0), dict(grid=None), dict(o=0), dict(v=0), dict(x=0), dict(c=0), dict(B=0), dict(B=-3), dict(N=1), dict(n_in=nan), dict(eps=nan),
                dict(t=T + 4), dict(x=X + 8), dict(grid=_lib.Grid.make([1, 8, 8], [-1] * 3, [1] * 3))):
        assert trace(**bad) == -1 and b"rnerf_scene_trace" in lib.rnerf_last_error(), bad
    huge = _lib.Grid.make([4, 2 ** 20, 64], [-1] * 3, [1] * 3)                  # a row stride of 2^30 bytes: what rnerf_march refuses
    assert trace(grid=huge) == -1
    assert lib.rnerf_march(p(T), ctypes.byref(huge), p(O), p(V), 4, 2.0, 6.0, 8, p(X), p(X), None, None, None) == -1

    alb = (ctypes.c_double * 3)(0.1, 0.2, 0.3)

    def shade(x=X, c=C, H=4, W=4, K=2, env=ENV, E=4, a=alb, rgb=RGB, tr=TR, m=M):
        return lib.rnerf_scene_shade(p(x), p(c), H, W, K, p(env), E, 0.01, 1.0, a, p(rgb), p(tr), p(m), None)

    for bad in (dict(x=0), dict(c=0), dict(env=0), dict(a=None), dict(rgb=0), dict(tr=0), dict(m=0), dict(H=0), dict(W=0), dict(K=0), dict(E=0),
                dict(H=1 << 14, W=1 << 14, K=4), dict(H=1 << 20, W=1, K=1 << 12)):
        assert shade(**bad) == -1 and b"rnerf_scene_shade" in lib.rnerf_last_error(), bad


def test_pose_spherical_and_orbit_cameras():
    pytest.importorskip("torch")
    from samplenerfro_amd import scenes
    c = scenes.pose_spherical(0.0, -90.0, 4.0)
    assert c.shape == (4, 4) and c.dtype == F32
    assert np.abs(c[:3, 3] - [0, 0, 4]).max() < 1e-6
    assert np.abs(c[:3, :3] @ np.array([0, 0, -1], F32) - [0, 0, -1]).max() < 1e-6          # the Blender camera looks down its -z
    for n, radius, phis, seed in ((7, 4.0, (-30.0,), None), (5, 2.5, (-10.0, -60.0, 20.0), 3)):
        poses = scenes.orbit_cameras(n, radius, phis, seed=seed)
        assert poses.shape == (n, 4, 4) and poses.dtype == F32
        for m in poses.astype(np.float64):
            r, t = m[:3, :3], m[:3, 3]
            assert np.abs(r.T @ r - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(r) - 1.0) < 1e-6
            assert abs(np.linalg.norm(t) - radius) < 1e-5
            assert np.abs(np.cross(r @ [0, 0, -1.0], -t / radius)).max() < 1e-6 and (r @ [0, 0, -1.0]) @ (-t) > 0      # the axis passes through the origin
            assert np.array_equal(m[3], [0, 0, 0, 1])
        az = np.degrees(np.arctan2(poses[:, 1, 3], poses[:, 0, 3]))
        gaps = np.sort(np.diff(np.sort(az)))
        assert np.abs(gaps - 360.0 / n).max() < 1e-3                                      # evenly spaced
    assert not np.array_equal(scenes.orbit_cameras(4, 4.0, (-30.0,), seed=0), scenes.orbit_cameras(4, 4.0, (-30.0,), seed=1))


def test_procedural_env_is_deterministic_and_seeded():
    pytest.importorskip("torch")
    from samplenerfro_amd import scenes
    a, b, c = scenes.procedural_env(16, 3), scenes.procedural_env(16, 3), scenes.procedural_env(16, 4)
    assert a.shape == (6, 16, 16, 3) and a.dtype == F32 and a.flags["C_CONTIGUOUS"]
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert 0.0 <= a.min() and a.max() <= 1.0 and a.std() > 0.05
    assert scenes.procedural_env(1, 0).shape == (6, 1, 1, 3)


def test_cube_from_function_and_the_lookup_agree_on_the_faces():
    """A function that is constant per face comes back as that constant in every texel, and the restatement's lookup of a texel centre
    returns that texel: the two halves of the convention (cube_directions and rnerf_scene_shade's rule) are one convention."""
    pytest.importorskip("torch")
    from samplenerfro_amd import scenes
    colours = np.arange(18, dtype=np.float64).reshape(6, 3) / 20.0

    def per_face(d):
        face, _, _, _ = R.cube_face(d.reshape(-1, 3).astype(F32))
        return colours[face].reshape(d.shape)

    E = 5
    env = scenes.cube_from_function(per_face, E)
    assert env.shape == (6, E, E, 3) and env.dtype == F32
    for f in range(6):
        assert np.array_equal(env[f], np.broadcast_to(colours[f].astype(F32), (E, E, 3)))
    dirs = scenes.cube_directions(E)
    assert np.abs(np.linalg.norm(dirs, axis=-1) - 1.0).max() < 1e-12
    tex = np.random.default_rng(0).uniform(0, 1, (6, E, E, 3)).astype(F32)
    got = R.cube_lookup(tex, dirs.reshape(-1, 3).astype(F32)).reshape(tex.shape)
    assert np.abs(got - tex).max() < 1e-5                                               # a centre has weight ~0 or ~1 up to the rounding of s


def test_the_lookup_picks_the_documented_face():
    cases = {(1, 0, 0): 0, (-1, 0, 0): 1, (0, 1, 0): 2, (0, -1, 0): 3, (0, 0, 1): 4, (0, 0, -1): 5,            # on the axes
             (1, 1, 0): 0, (-1, 1, 0): 1, (1, -1, 0.5): 0, (1, 0, 1): 0, (-1, 0.2, -1): 1, (0, 1, 1): 2, (0.3, -1, 1): 3, (0, -1, -1): 3,      # edges: x before y before z
             (1, 1, 1): 0, (-1, -1, -1): 1, (-1, 1, 1): 1, (0.5, 0.5, 0.5): 0,                               # corners
             (0.5, 1, -1): 2, (0.5, -0.7, -0.7): 3, (0.1, 0.2, -0.3): 5}
    d = np.array(list(cases), F32)
    face, a, b, m = R.cube_face(d)
    assert face.tolist() == list(cases.values())
    for (x, y, z), f, ai, bi, mi in zip(d, face, a, b, m):
        want = {0: (y, z), 1: (z, x), 2: (x, y)}[f // 2]
        assert (ai, bi) == want and mi == max(abs(x), abs(y), abs(z))
    bad = np.array([(0, 0, 0), (-0.0, 0.0, -0.0), (np.nan, 1, 0), (1, np.nan, 0), (0, 1, np.nan)], F32)
    assert R.cube_face(bad)[0].tolist() == [-1] * len(bad)
    env = np.random.default_rng(1).uniform(0.2, 1, (6, 3, 3, 3)).astype(F32)
    assert np.array_equal(R.cube_lookup(env, bad), np.zeros((len(bad), 3), F32))
    # one infinite component is a direction like any other: (s, t) = (0, 0), the centre of its face; two have inf / inf for a face
    # coordinate, which no texel answers: black
    inf = np.array([(np.inf, 0, 0), (1, -np.inf, 0), (-3, 2, np.inf)], F32)
    assert R.cube_face(inf)[0].tolist() == [0, 3, 4]
    assert np.array_equal(R.cube_lookup(env, inf), env[[0, 3, 4], 1, 1])
    two = np.array([(np.inf, -np.inf, 1), (0, np.inf, np.inf)], F32)
    assert np.array_equal(R.cube_lookup(env, two), np.zeros((2, 3), F32))


def test_the_lookup_at_one_texel_returns_the_texel():
    env = np.random.default_rng(2).uniform(0, 1, (6, 1, 1, 3)).astype(F32)
    rng = np.random.default_rng(3)
    d = rng.standard_normal((200, 3)).astype(F32)
    face = R.cube_face(d)[0]
    assert set(face.tolist()) == set(range(6))
    assert np.array_equal(R.cube_lookup(env, d), env[face, 0, 0])


def test_the_restated_shade_is_a_box_filter_of_its_samples():
    """sigma = 0: rgb is the mean of the K x K looked-up colours, trans is exactly 1; sigma > 0 with every node inside and a black
    environment: the albedo weighted by 1 - T; the mask is the any() of the refracting counts."""
    H, W, K, E = 2, 3, 2, 4
    rng = np.random.default_rng(5)
    d = rng.standard_normal((H * K * W * K, 3)).astype(F32)
    x = np.concatenate([d, np.zeros((len(d), 1), F32)], 1)
    counts = np.zeros((2, len(d)), np.int32)
    counts[1, 5] = 3
    env = rng.uniform(0, 1, (6, E, E, 3)).astype(F32)
    rgb, trans, mask = R.shade(x, counts, H, W, K, env, 0.01, 0.0, (0.5, 0.5, 0.5))
    want = R.cube_lookup(env, d).reshape(H, K, W, K, 3).astype(np.float64).mean(axis=(1, 3))
    assert np.abs(rgb - want).max() < 1e-6 and np.array_equal(trans, np.ones((H, W), F32))
    assert mask.sum() == 255 and mask[0, 2] == 255                                        # fine pixel 5 = fine row 0, column 5 -> pixel (0, 2)
    counts[0] = 10
    rgb, trans, _ = R.shade(x, counts, H, W, K, np.zeros_like(env), 0.01, 2.0, (0.2, 0.4, 0.8))
    T = np.exp(-2.0 * 0.01 * 10)
    assert np.abs(trans - T).max() < 1e-6 and np.abs(rgb - (1 - T) * np.array([0.2, 0.4, 0.8])).max() < 1e-6
