"""Host side of the depth visualisations (no GPU): tests/helpers/vis_ref.py against scipy and matplotlib where they are installed and
against answers worked by hand, the committed colour list, the argument checks of rnerf_vis_depth / rnerf_vis_normals, and evaluate's
signature."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vis_ref                       # noqa: E402

EPS32 = np.float32(2.0 ** -23)


def test_convolution_equals_scipy():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    for shape in ((1, 1), (3, 5), (17, 9)):
        z = rng.standard_normal(shape)
        for k in vis_ref.normal_kernels() + (rng.standard_normal((3, 3)),):
            want = signal.convolve2d(z, k, mode="same")
            assert np.max(np.abs(vis_ref.convolve2d_same(z, k) - want)) <= 1e-15 * max(1.0, np.max(np.abs(want)))


def test_turbo_step_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    rng = np.random.default_rng(1)
    value = np.concatenate([rng.uniform(0, 1, 4000), np.arange(257) / 256.0, [0.0, 1.0, np.nextafter(1.0, 0.0)]]).reshape(-1, 1)
    for dtype in (np.float32, np.float64):
        v = value.astype(dtype)
        index = np.minimum((v * dtype(256)).astype(np.int64), 255)
        want = matplotlib.colormaps["turbo"](v)[..., :3]
        assert np.array_equal(vis_ref.turbo_table()[index], want)
    d = rng.uniform(2, 6, (9, 11)).astype(np.float32)               # and through visualize_depth: acc = 1, so rgb is the colour
    out = vis_ref.visualize_depth(d)
    assert np.array_equal(out["rgb"], matplotlib.colormaps["turbo"](out["value"])[..., :3])


def test_committed_table_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    assert np.array_equal(vis_ref.turbo_table(), np.asarray(matplotlib.colormaps["turbo"].colors, np.float64))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_turbo_table
    assert open(make_turbo_table.OUT).read() == make_turbo_table.render(matplotlib.colormaps["turbo"].colors)


def test_committed_table_is_a_colour_list():
    t = vis_ref.turbo_table()
    assert t.shape == (256, 3) and t.min() >= 0.0 and t.max() <= 1.0
    assert len({tuple(r) for r in t}) == 256                        # distinct rows: a colour names its entry
    assert np.allclose(t[0], [0.18995, 0.07176, 0.23217]) and np.allclose(t[255], [0.4796, 0.01583, 0.01055])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_sloped_plane_gives_the_analytic_normal(dtype):
    a, b = 0.75, -0.5                                              # exact in both dtypes
    r, c = np.meshgrid(np.arange(7), np.arange(9), indexing="ij")
    z = (a * c + b * r + 2.0).astype(dtype)
    n = vis_ref.depth_to_normals(z, dtype)
    want = np.array([-a, -b, 1.0]) / np.sqrt(1 + a * a + b * b)
    assert n.dtype == dtype and np.max(np.abs(n[1:-1, 1:-1] - want)) <= 4 * np.finfo(dtype).eps
    rgb, normals, s = vis_ref.visualize_normals(z, None, scaling=1.0, dtype=dtype)
    assert s == 1 and np.array_equal(normals, n) and np.max(np.abs(rgb - (n + 1) / 2)) <= np.finfo(dtype).eps


def test_zero_padding_at_the_border():
    ky, kx = vis_ref.normal_kernels()
    one = np.ones((4, 5))
    dy, dx = vis_ref.convolve2d_same(one, ky), vis_ref.convolve2d_same(one, kx)
    assert np.array_equal(dy[0], [-0.375, -0.5, -0.5, -0.5, -0.375]) and np.array_equal(dy[-1], -dy[0]) and not dy[1:-1].any()
    assert np.array_equal(dx[:, 0], [-0.375, -0.5, -0.5, -0.375]) and np.array_equal(dx[:, -1], -dx[:, 0]) and not dx[:, 1:-1].any()
    one[2, 2] = np.nan                                              # every tap is multiplied: the 3 x 3 footprint, in both
    want = np.zeros((4, 5), bool)
    want[1:4, 1:4] = True
    assert np.array_equal(np.isnan(vis_ref.convolve2d_same(one, ky)), want) and np.array_equal(np.isnan(vis_ref.convolve2d_same(one, kx)), want)
    rgb = vis_ref.visualize_normals(one, None, scaling=1.0)[0]
    assert np.all(rgb[want] == 1.0) and np.all(np.isfinite(rgb))


def test_sinebow_of_zero():
    assert np.max(np.abs(vis_ref.sinebow(0.0) - [1.0, 0.25, 0.25])) <= 1e-15
    assert np.max(np.abs(vis_ref.sinebow(np.float32(0), np.float32) - [1.0, 0.25, 0.25])) <= 3e-7
    assert np.max(np.abs(vis_ref.sinebow(1.0) - vis_ref.sinebow(0.0))) <= 1e-15          # cyclic


def test_nan_sorts_last():
    d = np.array([[np.nan, 3.0, -np.inf], [np.inf, np.nan, -2.0]], np.float32)
    acc = np.full(d.shape, 0.5, np.float32)
    near, far = vis_ref.auto_range(d, acc, 0, np.float32)
    assert near == -np.inf and np.isnan(far)
    near, far = vis_ref.auto_range(np.where(np.isnan(d), 1.0, d), acc, 0, np.float32)
    assert near == -np.inf and far == np.inf
    # acc' is 0 at a NaN depth, so the four real pixels carry the total: cum 0.5 1 1.5 2 2 2 over -inf -2 3 inf nan nan, kept within [0.5, 1.5]
    near, far = vis_ref.auto_range(d, acc, 0.25, np.float32)
    assert near == -np.inf and far == np.float32(3.0) + EPS32
    assert all(np.isnan(v) for v in vis_ref.auto_range(np.full((2, 2), np.nan), None, 0, np.float64))
    out = vis_ref.visualize_depth(d, acc)
    assert not out["value"].any() and np.all(out["rgb"][np.isnan(d)] == 1.0)


def test_six_pixels_with_equal_depths_across_each_threshold():
    """Worked by hand.  In depth order, equal depths by pixel index (pixel: depth, acc -> cum):
         2: 1, 1 -> 1 | 1: 2, 0.5 -> 1.5 | 3: 2, 1.5 -> 3 | 0: 4, 0.5 -> 3.5 | 5: 4, 3.5 -> 7 | 4: 5, 1 -> 8
    total 8, ignore_frac 0.25: kept iff 2 <= cum <= 6, i.e. pixels 3 and 0: near = 2 - eps, far = 4 + eps.  The run of 2s straddles
    the low threshold and the run of 4s the high one; with the 4s in the other order (pixel 5 first: cum 6.5, 7) neither is kept and
    far would be 2 + eps."""
    d = np.array([[4, 2, 1], [2, 5, 4]], np.float32)
    acc = np.array([[0.5, 0.5, 1], [1.5, 1, 3.5]], np.float32)
    for dtype in (np.float32, np.float64):
        near, far = vis_ref.auto_range(d, acc, 0.25, dtype)
        assert np.float32(near) == np.float32(2) - EPS32 and np.float32(far) == np.float32(4) + EPS32
    flipped = vis_ref.auto_range(d[::-1, ::-1], acc[::-1, ::-1], 0.25)
    assert np.float32(flipped[1]) == np.float32(2) + EPS32
    near, far = vis_ref.auto_range(d, acc, 0)
    assert np.float32(near) == np.float32(1) - EPS32 and np.float32(far) == np.float32(5) + EPS32
    assert all(np.isnan(v) for v in vis_ref.auto_range(d[:1, :1], None, 0.25))          # one pixel: cum 1 > 0.75, nothing kept


def test_given_bounds_and_the_modular_value():
    d = np.array([[0.25, 0.5, 1.0, 2.0]], np.float32)
    out = vis_ref.visualize_depth(d, None, near=0.5, far=1.0, curve_fn="identity")
    assert np.array_equal(out["range"], [0.5, 1.0]) and np.array_equal(out["value"], [[0.0, 0.0, 1.0, 1.0]])
    assert np.array_equal(out["index"], [[0, 0, 255, 255]])
    out = vis_ref.visualize_depth(-d, None, curve_fn="identity", modulus=0.75)
    assert np.allclose(out["value"], [[2 / 3, 1 / 3, 2 / 3, 1 / 3]])                      # floored: the sign of the divisor
    assert np.allclose(out["rgb"], vis_ref.sinebow(out["value"]))


def test_argument_errors_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    nan = float("nan")
    p = lambda a: ctypes.c_void_p(a)
    D, A, RGB, VAL, RNG, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000      # never dereferenced: every call fails first

    def depth(depth=D, acc=A, H=4, W=4, near=nan, far=nan, frac=0.0, curve=0, modulus=0.0, rgb=RGB, value=VAL, rng=RNG, ws=WS):
        return lib.rnerf_vis_depth(p(depth), p(acc), H, W, near, far, frac, curve, modulus, p(rgb), p(value), p(rng), p(ws), None)

    def normals(depth=D, acc=A, H=4, W=4, scaling=nan, rgb=RGB, nrm=VAL, ws=WS):
        return lib.rnerf_vis_normals(p(depth), p(acc), H, W, scaling, p(rgb), p(nrm), p(ws), None)

    cases = [(lambda: depth(depth=None), b"null"), (lambda: depth(rgb=None, value=None, rng=None), b"null"),
             (lambda: depth(H=0), b"H >= 1"), (lambda: depth(W=-3), b"W >= 1"), (lambda: depth(H=1 << 16, W=1 << 15), b"2^31"),
             (lambda: depth(frac=0.5), b"ignore_frac"), (lambda: depth(frac=-0.1), b"ignore_frac"), (lambda: depth(frac=nan), b"ignore_frac"),
             (lambda: depth(modulus=-1.0), b"modulus"), (lambda: depth(modulus=float("inf")), b"modulus"),
             (lambda: depth(curve=4), b"curve"), (lambda: depth(curve=-1), b"curve"),
             (lambda: depth(ws=None), b"workspace"), (lambda: depth(ws=WS + 8), b"aligned"), (lambda: depth(near=1.0, ws=None), b"workspace"),
             (lambda: depth(rgb=D + 16), b"overlaps"), (lambda: depth(value=A), b"overlaps"), (lambda: depth(rng=D + 60), b"overlaps"),
             (lambda: depth(value=RGB + 64), b"overlap"),
             (lambda: normals(depth=None), b"null"), (lambda: normals(rgb=None, nrm=None), b"null"), (lambda: normals(H=0), b"H >= 1"),
             (lambda: normals(H=1 << 16, W=1 << 15), b"2^31"), (lambda: normals(ws=None), b"workspace"), (lambda: normals(ws=WS + 4), b"aligned"),
             (lambda: normals(rgb=A + 32), b"overlaps"), (lambda: normals(nrm=RGB), b"overlaps")]
    for call, word in cases:
        assert call() == -1
        msg = lib.rnerf_last_error()
        assert msg.startswith(b"rnerf_vis_") and word in msg, (msg, word)
    assert lib.rnerf_vis_depth_workspace_bytes(0, 4, 0.0) == 0 and b"rnerf_vis_depth" in lib.rnerf_last_error()
    assert lib.rnerf_vis_depth_workspace_bytes(4, 4, 0.5) == 0 and b"ignore_frac" in lib.rnerf_last_error()
    assert lib.rnerf_vis_normals_workspace_bytes(4, 0) == 0 and b"rnerf_vis_normals" in lib.rnerf_last_error()
    small, sorting = lib.rnerf_vis_depth_workspace_bytes(800, 800, 0.0), lib.rnerf_vis_depth_workspace_bytes(800, 800, 0.05)
    assert 0 < small <= 4096 and 16 * 800 * 800 < sorting - small < 18 * 800 * 800
    assert 0 < lib.rnerf_vis_normals_workspace_bytes(800, 800) <= 16384
    assert _lib.VIS_CURVES == {"neg_log": 0, "identity": 1, "reciprocal": 2, "log": 3}


def test_evaluate_signature_and_curve_names():
    pytest.importorskip("torch")
    from samplenerfro_amd import evaluate, vis
    assert inspect.signature(evaluate.evaluate).parameters["vis_suite"].default is False
    assert vis.CURVES == vis_ref.CURVES
    sig = inspect.signature(vis.visualize_depth)
    assert list(sig.parameters) == ["depth", "acc", "near", "far", "ignore_frac", "curve_fn", "modulus", "colormap"]
    assert sig.parameters["curve_fn"].default == "neg_log" and sig.parameters["ignore_frac"].default == 0
    with pytest.raises(TypeError, match="neg_log.*identity.*reciprocal.*log"):
        vis.visualize_depth(np.ones((2, 2), np.float32), curve_fn=lambda x: x)


def test_the_fixture_is_what_the_helper_gives():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_vis_reference as M
    fix = np.load(M.OUT)
    now = M.build()
    assert sorted(fix.files) == sorted(now)
    for k, v in now.items():
        if v.dtype == np.uint8:
            assert np.array_equal(fix[k], v), k
        else:
            assert fix[k].shape == v.shape and np.allclose(fix[k], v, rtol=1e-12, atol=1e-14, equal_nan=True), k
    assert os.path.getsize(M.OUT) < 512 * 1024
    d, acc = M.range_case((130, 257))                                # what the range cases promise
    keys = np.where(np.isfinite(d), d, 1).view(np.uint32).reshape(-1)
    assert all(len(np.unique((keys >> s) & 255)) == 256 for s in (0, 8, 16)) and len(np.unique(keys >> 24)) > 200
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d < 0).any() and (acc == 0).any()
    assert np.array_equal(acc * 64, np.round(acc * 64))
