"""rnerf_vis_depth / rnerf_vis_normals / samplenerfro_amd.vis on the device against tests/helpers/vis_ref.py in float64
(tests/golden/vis_reference.npz for the small cases; inputs from tests/golden/make_vis_reference.py).

Ranges: bit for bit (the inputs make every sum and threshold exact).  value, the depth_mod colours and the normals' colours: the float32
rule of tests/test_gpu_flip.py, max|gpu - f64| <= 4 max|f32 - f64| + 1e-6 with vis_ref in float32 as the floor.  Turbo colours: the
entry recovered from the colour differs from float64's by at most 1 on at most 1 % of the pixels (the float32 helper differs on none of
them for these inputs), and where it agrees the colour is the list's to 1e-6; blended with a fractional acc, also 1e-6: three float32
roundings at magnitude <= 1 and the entry's own, under 2.5e-7.

Measured on an MI355X (ratio = error / floor): see DESIGN.md 3.12."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_vis_reference as M       # noqa: E402
import vis_ref                       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
EPS32 = F32(2.0 ** -23)
IDS = [M.name(s) for s in M.SHAPES]


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def fix():
    return np.load(M.OUT)


_cache = {}


def ref64(shape, fix, key):
    """The float64 plane `key` of the smooth / mod case: from the fixture, or from the helper (once) for the largest shape."""
    k = f"{M.name(shape)}/{key}"
    if k in fix.files:
        return fix[k]
    if shape not in _cache:
        _cache[shape] = {kk: v for kk, v in M.outputs(shape).items()}
        d, acc = M.smooth_case(shape)
        dep = vis_ref.visualize_depth(d, acc, **M.bounds(shape))
        md, macc = M.mod_case(shape)
        _cache[shape].update(value=dep["value"], depth=dep["rgb"], depth_mod=vis_ref.visualize_depth(d, acc, modulus=0.1)["rgb"],
                             depth_normals=vis_ref.visualize_normals(d, acc)[0], mod_value=vis_ref.visualize_depth(md, macc, modulus=0.1)["value"])
    return _cache[shape][key]


def f32_rule(gpu, f64, f32, what):
    assert gpu.shape == f64.shape and not np.isnan(gpu).any() and not np.isnan(f64).any(), what
    e_gpu, e_32 = float(np.max(np.abs(gpu - f64))), float(np.max(np.abs(f32.astype(np.float64) - f64)))
    print(f"{what}: error {e_gpu:.3g} (float32 {e_32:.3g}, ratio {e_gpu / max(e_32, 1e-30):.3g})")
    assert e_gpu <= 4 * e_32 + 1e-6, f"{what}: error {e_gpu:.3g} vs float32's {e_32:.3g}"


def same_bits(got, want):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))


def gpu_range(d, acc, frac, **kw):
    from samplenerfro_amd import ops
    return ops.vis_depth(T(d), T(acc), ignore_frac=frac, want_rgb=False, want_range=True, **kw)[2].cpu().numpy()


@pytest.mark.parametrize("frac", M.FRACS)
@pytest.mark.parametrize("shape", M.SHAPES, ids=IDS)
def test_range_is_exact(shape, frac, fix):
    d, acc = M.range_case(shape)
    want = fix[f"{M.name(shape)}/range_{frac}"]
    got = gpu_range(d, acc, frac)
    print(f"{M.name(shape)} ignore_frac {frac}: range {got} (float64 {want})")
    assert same_bits(got, want.astype(F32)), (got, want)
    assert same_bits(got, np.array(vis_ref.auto_range(d, acc, frac, F32)))
    assert same_bits(gpu_range(d, None, frac), np.array(vis_ref.auto_range(d, None, frac)).astype(F32))      # acc = None: all ones
    # a given bound passes through unchanged and the other is still found; both given: nothing is computed
    assert same_bits(gpu_range(d, acc, frac, near=1.25), [1.25, want[1]])
    assert same_bits(gpu_range(d, acc, frac, far=-7.5), [want[0], -7.5])
    assert same_bits(gpu_range(d, acc, frac, near=3.0, far=0.1), [3.0, F32(0.1)])


def test_six_pixels_worked_by_hand():
    """tests/test_vis_host.py::test_six_pixels_with_equal_depths_across_each_threshold: the stable order decides the far bound."""
    d = np.array([[4, 2, 1], [2, 5, 4]], F32)
    acc = np.array([[0.5, 0.5, 1], [1.5, 1, 3.5]], F32)
    assert same_bits(gpu_range(d, acc, 0.25), [F32(2) - EPS32, F32(4) + EPS32])
    assert same_bits(gpu_range(d[::-1, ::-1], acc[::-1, ::-1], 0.25), [F32(2) - EPS32, F32(2) + EPS32])
    assert same_bits(gpu_range(d, acc, 0.0), [F32(1) - EPS32, F32(5) + EPS32])
    assert same_bits(gpu_range(d[:1, :1], None, 0.25), [np.nan, np.nan])                  # nothing kept


@pytest.mark.parametrize("shape", M.SHAPES, ids=IDS)
def test_value_and_colours_under_the_float32_rule(shape, fix):
    from samplenerfro_amd import ops
    d, acc = M.smooth_case(shape)
    what = M.name(shape)
    b = M.bounds(shape)
    value = N(ops.vis_depth(T(d), T(acc), want_rgb=False, want_value=True, **b)[1])
    f32_rule(value, ref64(shape, fix, "value"), vis_ref.visualize_depth(d, acc, dtype=F32, **b)["value"], f"{what} value")
    md, macc = M.mod_case(shape)
    mod_value = N(ops.vis_depth(T(md), T(macc), modulus=0.1, want_rgb=False, want_value=True)[1])
    f32_rule(mod_value, ref64(shape, fix, "mod_value"), vis_ref.visualize_depth(md, macc, modulus=0.1, dtype=F32)["value"], f"{what} modular value")
    mod = N(ops.vis_depth(T(d), T(acc), modulus=0.1)[0])
    f32_rule(mod, ref64(shape, fix, "depth_mod"), vis_ref.visualize_depth(d, acc, modulus=0.1, dtype=F32)["rgb"], f"{what} depth_mod")
    nrm = N(ops.vis_normals(T(d), T(acc))[0])
    f32_rule(nrm, ref64(shape, fix, "depth_normals"), vis_ref.visualize_normals(d, acc, dtype=F32)[0], f"{what} depth_normals")


@pytest.mark.parametrize("curve", ["identity", "reciprocal", "log"])
def test_the_other_curves(curve):
    from samplenerfro_amd import ops
    d, acc = M.smooth_case((37, 53))
    value = N(ops.vis_depth(T(d), T(acc), curve=curve, want_rgb=False, want_value=True)[1])
    f32_rule(value, vis_ref.visualize_depth(d, acc, curve_fn=curve)["value"], vis_ref.visualize_depth(d, acc, curve_fn=curve, dtype=F32)["value"],
             f"{curve} value")


def table_index(rgb):
    """The entry of the colour list nearest to each pixel's colour, and the distance to it."""
    t = vis_ref.turbo_table()
    dist = np.max(np.abs(rgb.reshape(-1, 1, 3) - t[None]), -1)
    idx = np.argmin(dist, -1)
    return idx.reshape(rgb.shape[:-1]), dist[np.arange(idx.size), idx].reshape(rgb.shape[:-1])


@pytest.mark.parametrize("shape", M.SHAPES, ids=IDS)
def test_turbo_colours(shape, fix):
    from samplenerfro_amd import ops
    d, acc = M.smooth_case(shape)
    want = fix[f"{M.name(shape)}/index"].astype(np.int64)
    rgb = N(ops.vis_depth(T(d), None, **M.bounds(shape))[0])                             # acc = 1: the colour itself
    idx, dist = table_index(rgb)
    assert float(dist.max()) <= 1e-6                                                     # every colour is an entry of the list
    off = np.abs(idx - want)
    print(f"{M.name(shape)}: turbo entry differs from float64's on {int((off > 0).sum())} of {off.size} pixels (max {int(off.max())})")
    assert off.max() <= 1 and (off > 0).sum() <= 0.01 * off.size
    agree = off == 0
    assert float(np.max(np.abs(rgb[agree] - vis_ref.turbo_table()[want[agree]]), initial=0.0)) <= 1e-6
    blend = N(ops.vis_depth(T(d), T(acc), **M.bounds(shape))[0])                         # fractional acc: colour * acc + (1 - acc)
    ref = vis_ref.turbo_table()[want] * acc[..., None].astype(np.float64) + (1 - acc[..., None].astype(np.float64))
    assert float(np.max(np.abs(blend[agree] - ref[agree]), initial=0.0)) <= 1e-6
    if f"{M.name(shape)}/depth" in fix.files:
        assert np.array_equal(ref, fix[f"{M.name(shape)}/depth"])


def test_nan_rules():
    from samplenerfro_amd import ops
    d, acc = M.smooth_case((37, 53))
    d = d.copy()
    d[5, 7] = d[36, 52] = d[0, 20] = np.nan
    nan = np.isnan(d)
    rgb, value, rng = ops.vis_depth(T(d), T(acc), want_value=True, want_range=True)
    rng = rng.cpu().numpy()
    assert rng[0] == F32(np.nanmin(d)) - EPS32 and np.isnan(rng[1])                       # NaN sorts last: it is the far bound
    assert not N(value).any()                                                            # min(n, NaN) = NaN -> nan_to_num -> 0
    want = vis_ref.visualize_depth(d, acc)
    assert np.max(np.abs(N(rgb) - want["rgb"])) <= 1e-6 and np.all(N(rgb)[nan] == 1.0)    # white where acc' = 0
    rgb, value, _ = ops.vis_depth(T(d), T(acc), modulus=0.1, want_value=True)            # depth_mod keeps NaN
    assert np.array_equal(np.isnan(N(value)), nan) and np.array_equal(np.isnan(N(rgb)), np.repeat(nan[..., None], 3, -1))
    foot = np.zeros(d.shape, bool)
    for r, c in zip(*np.nonzero(nan)):
        foot[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = True
    rgb, normals = ops.vis_normals(T(d), None, want_normals=True)
    normals, rgb = N(normals), N(rgb)
    assert np.array_equal(np.isnan(normals[..., 0]), foot) and np.array_equal(np.isnan(normals[..., 1]), foot) and np.array_equal(np.isnan(normals[..., 2]), foot)
    assert np.all(rgb[foot] == 1.0) and not np.isnan(rgb).any()
    want_rgb, want_n, s = vis_ref.visualize_normals(d, None)
    assert np.max(np.abs(rgb - want_rgb)) <= 4 * float(np.max(np.abs(vis_ref.visualize_normals(d, None, dtype=F32)[0] - want_rgb))) + 1e-6
    blended = N(ops.vis_normals(T(d), T(acc))[0])                                        # the raw acc, also at a NaN depth
    a = acc[..., None].astype(np.float64)
    assert np.max(np.abs(blended - (rgb * a + (1 - a)))) <= 1e-6
    flat = np.full((9, 12), 3.5, F32)                                                    # equal depths: variance 0, infinite scaling
    rgb, normals = ops.vis_normals(T(flat), None, want_normals=True)
    assert bool(torch.isnan(normals).all()) and bool((rgb == 1).all())
    allnan = np.full((4, 6), np.nan, F32)
    rng = ops.vis_depth(T(allnan), None, want_rgb=False, want_range=True)[2].cpu().numpy()
    assert np.isnan(rng).all()
    assert bool((ops.vis_normals(T(allnan), None)[0] == 1).all())


def test_two_runs_give_identical_bytes():
    from samplenerfro_amd import ops, vis
    d, acc = M.range_case((130, 257))
    d = np.where(np.isinf(d), F32(3), d)
    td, ta = T(np.abs(d)), T(acc)
    calls = [lambda: ops.vis_depth(td, ta, want_value=True, want_range=True), lambda: ops.vis_depth(td, ta, modulus=0.1, want_value=True),
             lambda: ops.vis_depth(td, ta, ignore_frac=0.05, want_value=True, want_range=True),
             lambda: ops.vis_depth(td, ta, ignore_frac=0.25, near=0.5, curve="log", want_range=True),
             lambda: ops.vis_normals(td, ta, want_normals=True), lambda: tuple(vis.visualize_suite(td, ta).values())]
    for call in calls:
        one, two = call(), call()
        for x, y in zip(one, two):
            assert (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_suite_equals_the_three_calls_and_uploads():
    from samplenerfro_amd import vis
    d, acc = M.smooth_case((37, 53))
    suite = vis.visualize_suite(T(d), T(acc))
    assert sorted(suite) == ["depth", "depth_mod", "depth_normals"]
    for v in suite.values():
        assert v.is_cuda and v.dtype == torch.float32 and v.shape == (37, 53, 3)
    assert torch.equal(suite["depth"], vis.visualize_depth(T(d), T(acc)))
    assert torch.equal(suite["depth_mod"], vis.visualize_depth(T(d), T(acc), modulus=0.1))
    assert torch.equal(suite["depth_normals"], vis.visualize_normals(T(d), T(acc)))
    up = vis.visualize_suite(d, torch.from_numpy(acc))                                   # numpy + CPU tensor are uploaded
    assert all(torch.equal(up[k], suite[k]) for k in suite)
    assert torch.equal(vis.visualize_depth(d.astype(np.float64), T(acc), near=0, far=None), suite["depth"])      # 0 is "automatic" too
    assert torch.equal(vis.visualize_depth(T(d)), vis.visualize_depth(T(d), np.ones_like(d)))
    n = vis.depth_to_normals(d)
    assert n.shape == (37, 53, 3) and np.max(np.abs(N(n) - vis_ref.depth_to_normals(d))) <= 1e-6
    h = np.linspace(-1, 2, 50, dtype=F32)
    assert np.max(np.abs(N(vis.sinebow(h)) - vis_ref.sinebow(h))) <= 5e-6          # float32 arguments up to 10: half an ulp there is 5e-7
    with pytest.raises(ValueError):
        vis.visualize_depth(T(d), T(acc[:5]))
    with pytest.raises(ValueError):
        vis.visualize_depth(T(d), curve_fn="sqrt")
    from samplenerfro_amd import _lib
    with pytest.raises(_lib.RnerfError, match="ignore_frac"):
        vis.visualize_depth(T(d), ignore_frac=0.5)


def test_a_callable_colormap_sees_the_value_plane():
    from samplenerfro_amd import ops, vis
    d, acc = M.smooth_case((37, 53))
    seen = []

    def cmap(v):
        seen.append(v)
        return torch.stack([v, 1 - v, v * 0 + 0.25, v], -1)                              # four channels: the first three count

    rgb = vis.visualize_depth(T(d), T(acc), ignore_frac=0.125, colormap=cmap)
    value = ops.vis_depth(T(d), T(acc), ignore_frac=0.125, want_rgb=False, want_value=True)[1]
    assert len(seen) == 1 and seen[0].is_cuda and torch.equal(seen[0], value)
    a = T(acc)[..., None]
    assert torch.equal(rgb, torch.stack([value, 1 - value, value * 0 + 0.25], -1) * a + (1 - a))
    via = vis.visualize_depth(T(d), T(acc), modulus=0.1, colormap=vis.sinebow)           # the built-in map, applied outside
    assert float((via - vis.visualize_depth(T(d), T(acc), modulus=0.1)).abs().max()) <= 2e-6
    with pytest.raises(ValueError):
        vis.visualize_depth(T(d), colormap=lambda v: v)


def test_800x800_properties():
    from samplenerfro_amd import ops, vis
    d, acc = M._range_inputs((800, 800), 5)                                              # 157 sort blocks; sums exact as in the small cases
    for frac in (0.0, 0.125):
        assert same_bits(gpu_range(d, acc, frac), np.array(vis_ref.auto_range(d, acc, frac)).astype(F32))
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.linspace(-1, 1, 800), np.linspace(-1, 1, 800), indexing="ij")
    d = (4 + np.sin(3 * xx) * np.cos(2 * yy) + 0.01 * rng.standard_normal((800, 800))).astype(F32)
    acc = np.clip(1.2 - (xx ** 2 + yy ** 2), 0, 1).astype(F32)
    suite = vis.visualize_suite(d, acc)
    for v in suite.values():
        assert v.shape == (800, 800, 3) and float(v.min()) >= 0.0 and float(v.max()) <= 1.0
    _, value, r = ops.vis_depth(T(d), T(acc), want_value=True, want_range=True)
    assert float(value.min()) >= 0.0 and float(value.max()) <= 1.0 and float(r[0]) == float(F32(d.min()) - EPS32) and float(r[1]) == float(F32(d.max()) + EPS32)
    assert float(value.flatten()[int(np.argmin(d))]) == float(value.max())              # neg_log: the nearest pixel has the highest value
    normals = ops.vis_normals(T(d), None, want_rgb=False, want_normals=True)[1]
    assert float((normals.double().pow(2).sum(-1) - 1).abs().max()) <= 1e-6 and float(normals[..., 2].min()) > 0
    want = vis_ref.visualize_normals(d, acc)[0]
    f32_rule(N(suite["depth_normals"]), want, vis_ref.visualize_normals(d, acc, dtype=F32)[0], "800x800 depth_normals")


def test_the_suite_does_not_synchronise():
    from samplenerfro_amd import vis
    d, acc = M.smooth_case((130, 257))
    td, ta = T(d), T(acc)
    first = vis.visualize_suite(td, ta)
    torch.cuda.synchronize()
    torch.cuda._sleep(50_000_000)                      # keep the stream busy for tens of milliseconds
    s = vis.visualize_suite(td, ta)
    done = torch.cuda.Event()
    done.record()
    assert not done.query(), "visualize_suite returned after the stream drained: it synchronised"
    torch.cuda.synchronize()
    assert all(torch.equal(s[k], first[k]) for k in s)
