"""rnerf_path_summary and rnerf_path_plot on the device, bit for bit against tests/helpers/paths_ref.py: the summary on seeded records
with every edge case of the refracting rule and on the device's own march (plain and stage "all"), the plot on hand-made polylines with
every kind of segment and overlap, and the Python layer (view_maps chunked, trace_pixels against model.forward's taps, plot_paths and
write_plots) on top."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import paths_ref as R               # noqa: E402
import paths_scene as PS            # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
T = PS.T


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == F32 else a


def check_summary(pd, dr, ior, grad_eps=1e-3):
    """The device's summary of the records equals the restatement's, every bit; -> the restatement's (nodes, maps)."""
    from samplenerfro_amd import ops
    nodes, maps = ops.path_summary(T(pd), T(dr), T(ior), grad_eps)
    want_nodes, want_maps = R.summary(pd, dr, ior, grad_eps)
    assert nodes.dtype == torch.int32 and maps.dtype == torch.float32
    assert tuple(nodes.shape) == want_nodes.shape and tuple(maps.shape) == want_maps.shape
    for name, g, w in zip(("count", "first", "last"), nodes.cpu().numpy(), want_nodes):
        assert np.array_equal(g, w), (name, np.flatnonzero(g != w)[:8])
    for name, g, w in zip(("bend", "optical"), bits(maps), bits(want_maps)):
        assert np.array_equal(g, w), (name, np.flatnonzero(g != w)[:8])
    return want_nodes, want_maps


# ---- the summary on seeded records ----------------------------------------------------------------------------------------------------
def synthetic_records(N, B, seed):
    """Rows by r % 8 (B > 1): 0 no refracting node, 1 every node, 2 a norm of exactly float32(1e-3), 3 NaN gradients, 4 only node 0,
    5 only node N - 1, 6 and 7 gradients spread around the threshold."""
    rng = np.random.default_rng(seed)
    pd = np.cumsum(rng.uniform(-0.1, 0.1, (N, B, 4)), axis=0).astype(F32)
    dr = rng.standard_normal((N, B, 4))
    dr = (dr / np.linalg.norm(dr[..., :3], axis=-1, keepdims=True)).astype(F32)
    dr[..., 3] = 0
    ior = np.empty((N, B, 4), F32)
    ior[..., 0] = rng.uniform(1.0, 1.5, (N, B))
    ior[..., 1:] = (rng.standard_normal((N, B, 3)) * 10.0 ** rng.uniform(-4.5, -1.5, (N, B, 1))).astype(F32)
    kind = np.arange(B) % 8 if B > 1 else np.array([6])
    t = F32(1e-3)
    for r in range(B):
        k = kind[r]
        if k == 0:
            ior[:, r, 1:] = 0
        elif k == 1:
            ior[:, r, 1:] = rng.uniform(0.01, 1.0, (N, 3))
        elif k == 2:
            ior[:, r, 1:] = 0
            ior[:, r, 1 + r % 3] = t
            ior[N // 2:, r, 1 + r % 3] = -t
        elif k == 3:
            ior[:, r, 1:] = 0
            ior[::2, r, 2] = np.nan
            ior[1, r, 1:] = (np.nan, 1.0, 1.0)
        elif k == 4:
            ior[:, r, 1:] = 0
            ior[0, r, 1:] = (0.0, 0.5, 0.0)
        elif k == 5:
            ior[:, r, 1:] = 0
            ior[N - 1, r, 1:] = (0.0, 0.0, -0.5)
    return pd, dr, ior, kind


# (13, 70): two waves, the second ragged; N - 1 = 12 segments = one batch of 8 nodes in flight and a remainder of 4.  (2, 70), (13, 1):
# the smallest.  (9, 3): exactly one batch; (17, 5): two batches, the second loaded ahead, no remainder; (41, 70): five batches.
@pytest.mark.parametrize("N,B", [(13, 70), (13, 1), (2, 70), (9, 3), (17, 5), (41, 70)])
def test_summary_on_seeded_records(N, B):
    pd, dr, ior, kind = synthetic_records(N, B, seed=100 * N + B)
    t = F32(1e-3)
    assert np.sqrt(t * t) == t                                                   # the threshold row sits exactly on the threshold
    nodes, maps = check_summary(pd, dr, ior)
    for r in range(B):
        want = {0: [0, -1, -1], 1: [N, 0, N - 1], 2: [0, -1, -1], 3: [0, -1, -1], 4: [1, 0, 0], 5: [1, N - 1, N - 1]}.get(int(kind[r]))
        if want is not None:
            assert nodes[:, r].tolist() == want, (r, kind[r])
    if B > 8:
        assert 0 < nodes[0, 6] < N                                               # the random rows have both kinds of node
    assert np.isfinite(maps).all()


def test_summary_takes_the_threshold_as_float32_and_another_one():
    pd, dr, ior, _ = synthetic_records(13, 70, seed=7)
    a, _ = check_summary(pd, dr, ior, grad_eps=1e-3)
    b, _ = check_summary(pd, dr, ior, grad_eps=3e-2)
    assert (b[0] <= a[0]).all() and (b[0] < a[0]).any()
    ior[:, 2, 1:] = 0
    ior[:, 2, 1] = np.nextafter(F32(1e-3), F32(1))                               # one float32 above the threshold: every node counts
    assert check_summary(pd, dr, ior)[0][:, 2].tolist() == [13, 0, 12]


# ---- the summary on the device's own march ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ball():
    from samplenerfro_amd import _lib, ops
    b = PS.ball()
    spec = _lib.Grid.make(b["ndim"], b["nmin"], b["nmax"])
    b.update(spec=spec, table=ops.grid_build_table(T(b["grid"]), spec))
    return b


def so3_flat():
    from samplenerfro_amd import models, synthetic as syn
    rng = np.random.default_rng(21)
    flat = syn.init_mlp_flat(rng, models.SO3_MLP_SHAPES, 0.05)
    flat[-(128 * 3 + 3):-3] = (0.1 * rng.standard_normal(128 * 3)).astype(F32)   # a head that turns the gradient visibly
    return flat


def march_records(ball, stage):
    from samplenerfro_amd import ops
    o, d = T(ball["o"]), T(ball["d"])
    if stage == "all":
        pd, dr, ior = ops.march_all(ball["table"], ball["spec"], T(so3_flat()), o, d, 2.0, 6.0, PS.BALL_N, 1.0, want_ior=True)
    else:
        pd, dr, ior, _ = ops.march(ball["table"], ball["spec"], o, d, 2.0, 6.0, PS.BALL_N, want_ior=True)
    return pd.cpu().numpy(), dr.cpu().numpy(), ior.cpu().numpy()


@pytest.mark.parametrize("stage", ["radiance", "all"])
def test_summary_on_the_devices_own_march(ball, stage):
    pd, dr, ior = march_records(ball, stage)                                     # read back: input of the restatement, not code under test
    nodes, maps = check_summary(pd, dr, ior)
    hit = nodes[0] > 0
    assert 10 < hit.sum() < PS.BALL_B                                            # some rays meet the ball, some pass it
    assert (maps[1][hit] > 0).all() and (maps[0][hit] > 0).any()
    assert (nodes[1][hit] <= nodes[2][hit]).all() and (nodes[1][~hit] == -1).all() and (nodes[2][~hit] == -1).all()


# ---- the plot on hand-made polylines -----------------------------------------------------------------------------------------------------
SIZE = 37
HAND = [[10.0, 0.0, 0.0, 18.5], [0.0, 0.0, -10.0, 18.5]]                         # x to the right, z up, 10 pixels per unit, the origin in the middle


def polylines():
    """pd [N, 5, 4] in units of the hand-written panel (pixel = 10 x + 18.5, 18.5 - 10 z) and ior [N, 5, 4].
    ray 0: from the middle out and back in all 8 octants, along both axes, and zero-length segments; refracting nodes on it.
    ray 1: in and out across each of the four borders, and one segment wholly outside.
    ray 2: a node at 1e30 (skipped with both its segments), one just below the 2^30 limit (clipped), a NaN node.
    rays 3 and 4: the same polyline twice."""
    star = []
    for dx, dz in ((1.2, 0.5), (0.5, 1.2), (-0.5, 1.2), (-1.2, 0.5), (-1.2, -0.5), (-0.5, -1.2), (0.5, -1.2), (1.2, -0.5), (1.0, 0.0), (0.0, 1.0),
                   (-1.3, 0.0), (0.0, -1.3)):
        star += [(0.0, 0.0), (dx, dz)]
    star += [(0.0, 0.0), (0.0, 0.0), (0.0, 0.0)]
    cross = [(-3.0, 0.6), (-1.0, 0.7), (-1.1, 3.0), (1.0, 1.0), (3.1, 0.9), (0.9, -1.0), (1.0, -3.2), (-2.5, -2.6), (-2.5, 2.8), (-4.0, -4.0), (-2.0, -5.0)]
    near_limit = F32((2.0 ** 30 - 1000.0) / 10.0)
    wild = [(0.3, -0.3), (1e30, 0.0), (0.5, 0.5), (float(near_limit), 0.4), (-0.4, 0.4), (float("nan"), 0.0), (-0.6, -0.6), (-0.6, -1.0)]
    twin = [(-1.5, -1.5), (-0.2, 1.4), (1.5, -1.5), (-1.5, 0.3)]
    rows = [star, cross, wild, twin, twin]
    N = max(len(r) for r in rows)
    pd = np.zeros((N, len(rows), 4), F32)
    for r, pts in enumerate(rows):
        pts = pts + [pts[-1]] * (N - len(pts))
        pd[:, r, 0] = [p[0] for p in pts]
        pd[:, r, 2] = [p[1] for p in pts]
        pd[:, r, 1] = 0.1 * r + 0.03 * np.arange(N)                               # depth: the other views differ from the hand-written one
    ior = np.ones((N, len(rows), 4), F32)
    ior[:, :, 1:] = 0
    ior[1, 0, 1:] = (0.5, 0.0, 0.0)                                              # a marker on a path end, beside the box edge
    ior[0, 0, 1:] = (0.0, 0.2, 0.0)                                              # in the middle, over the paths of every octant
    ior[2, 3, 1:] = (0.0, 0.0, 0.3)
    ior[3, 2, 1:] = (1.0, 0.0, 0.0)                                              # on the node near the limit: outside every panel
    ior[1, 2, 1:] = (1.0, 0.0, 0.0)                                              # on the node that cannot be drawn
    ior[5, 1, 1:] = (F32(1e-3), 0.0, 0.0)                                        # on the threshold: no marker
    return pd, ior


def panels():
    from samplenerfro_amd import paths
    return np.concatenate([paths.view_matrices([0.0, 0.2, 0.0], 2.6, SIZE), np.asarray([HAND], np.float64)], 0)


BOX = (-1.25, -0.5, -1.25, 1.25, 1.0, 1.25)
PLOT_CASES = {
    "all_layers": dict(rays=[0, 1, 2, 3, 4], ior=True, floor_z=-1.25, box=BOX),
    "bare": dict(rays=[0, 1, 2, 3, 4], ior=False, floor_z=float("nan"), box=None),
    "one_ray": dict(rays=[0], ior=True, floor_z=-0.7, box=BOX),
    "indices_outside": dict(rays=[3, 99, -1, 0], ior=True, floor_z=float("nan"), box=BOX),
}


def run_plot(case, pd, ior):
    from samplenerfro_amd import ops, paths
    rays = np.asarray(case["rays"], np.int32)
    rgb = paths.ray_colours(len(rays))
    pan = panels()
    args = dict(box=case["box"], floor_z=case["floor_z"])
    got = ops.path_plot(T(pd), T(ior) if case["ior"] else None, T(rays), T(rgb), pan, SIZE, **args)
    want = R.plot(pd, ior if case["ior"] else None, rays, rgb, pan, SIZE, **args)
    return got, want, R.plot_keys(pd, ior if case["ior"] else None, rays, pan, SIZE, **args)


@pytest.mark.parametrize("name", sorted(PLOT_CASES))
def test_plot_on_hand_made_polylines(name):
    pd, ior = polylines()
    got, want, keys = run_plot(PLOT_CASES[name], pd, ior)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, SIZE, SIZE, 3)
    g = got.cpu().numpy()
    assert np.array_equal(g, want), [(p, int((g[p] != want[p]).any(-1).sum())) for p in range(5)]
    layers = set(np.unique(keys >> 28).tolist())
    if name == "all_layers":
        assert layers == {0, R.BOX, R.SHADOW, R.PATH, R.MARKER}
        again, _, _ = run_plot(PLOT_CASES[name], pd, ior)
        assert torch.equal(again, got)                                           # an integer maximum: the same bytes on every run
        hand = keys[4]
        assert hand[18, 18] == R.MARKER << 28 | 0                                # the marker in the middle lies over every path through it
        assert hand[13, 30] == R.MARKER << 28 | 0 and (hand[12:15, 29:32] >> 28 == R.MARKER).all()      # node (1.2, 0.5): pixel (30, 13)
        # rays 3 and 4 differ in y alone, which this panel does not see: of two equal polylines the higher slot shows
        assert not (hand == (R.PATH << 28 | 3)).any() and (hand == (R.PATH << 28 | 4)).any()
        assert not (hand == (R.SHADOW << 28 | 3)).any() and (hand == (R.SHADOW << 28 | 4)).any()
        assert (keys[:4] == (R.PATH << 28 | 3)).any()                            # the other views tell them apart
        assert (hand[:, 0] >> 28 != 0).any() and (hand[0, :] >> 28 != 0).any() and (hand[:, -1] >> 28 != 0).any() and (hand[-1, :] >> 28 != 0).any()
        assert (hand[6, :] >> 28 == R.BOX).sum() > 10                            # the box's upper edge z = 1.25: row floor(18.5 - 12.5) = 6
        assert hand[14, 18:SIZE].tolist().count(R.PATH << 28 | 2) > 10           # the segment to the node near the limit, cut at the border
    elif name == "bare":
        assert layers == {0, R.PATH}
    elif name == "one_ray":
        assert layers == {0, R.BOX, R.SHADOW, R.PATH, R.MARKER} and set(np.unique(keys & 0x0FFFFFFF)[np.unique(keys & 0x0FFFFFFF) > 11]) == set()
    else:
        ids = set(np.unique(keys[keys >> 28 == R.PATH] & 0x0FFFFFFF).tolist())
        assert ids == {0, 3}                                                     # slots 1 and 2 hold indices outside [0, B): nothing drawn


def test_the_point_near_the_limit_is_drawable_and_the_one_beyond_is_not():
    pd, _ = polylines()
    assert R.pixel(HAND, pd[3, 2, :3]) is not None and R.pixel(HAND, pd[3, 2, :3])[0] > 2 ** 29
    assert R.pixel(HAND, pd[1, 2, :3]) is None and R.pixel(HAND, pd[5, 2, :3]) is None
    assert R.pixel(HAND, (F32(2.0 ** 30 / 10.0), 0.0, 0.0)) is None


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_plot_paths_and_write_plots_on_the_march(ball, tmp_path):
    from PIL import Image
    from samplenerfro_amd import paths
    pd, dr, ior = march_records(ball, "radiance")
    rays = [0, 5, 69, 33]
    loaded = set(sys.modules)
    box = ball["nmin"] + ball["nmax"]
    got = paths.plot_paths(T(pd), T(ior), rays, size=SIZE, frame="grid", box=box)
    side = 3.0
    pan = paths.view_matrices([0.0, 0.0, 0.0], side, SIZE)
    want = R.plot(pd, ior, rays, paths.ray_colours(4), pan, SIZE, box=box, floor_z=-1.5)
    assert np.array_equal(got.cpu().numpy(), want)
    assert len({tuple(c) for c in want.reshape(-1, 3).tolist()}) >= 5             # background, box, shadow, marker and at least one ray colour
    # frame="paths": centre, side and floor from the drawn positions (plot_path:32-35,54)
    pos = pd[:, rays, :3].reshape(-1, 3).astype(np.float64)
    center, side = pos.mean(0), float((pos.max(0) - pos.min(0)).max())
    got_p = paths.plot_paths(T(pd), None, torch.tensor(rays), size=SIZE, shadow=True)
    want_p = R.plot(pd, None, rays, paths.ray_colours(4), paths.view_matrices(center, side, SIZE), SIZE, floor_z=float(center[2] - side * 0.5))
    assert np.array_equal(got_p.cpu().numpy(), want_p)
    names = paths.write_plots(str(tmp_path), got)
    assert sorted(os.listdir(tmp_path)) == ["free.png", "front.png", "right.png", "top.png"]
    assert [os.path.basename(n) for n in names] == ["top.png", "right.png", "front.png", "free.png"]
    for n, panel in zip(names, want):
        assert np.array_equal(np.asarray(Image.open(n)), panel)
    assert not {"jax", "matplotlib", "cv2"} & {m.split(".")[0] for m in set(sys.modules) - loaded}      # none of them is needed
    with pytest.raises(ValueError):
        paths.plot_paths(T(pd), None, [PS.BALL_B], size=SIZE)
    with pytest.raises(ValueError):
        paths.plot_paths(T(pd), None, [0], size=7)


@pytest.fixture(scope="module")
def crop():
    return PS.example_crop()


def test_view_maps_equals_one_whole_march_at_every_chunk(crop):
    from samplenerfro_amd import paths
    from samplenerfro_amd.utils import Rays
    model, variables, rays = crop["model"], crop["variables"], crop["rays"]
    flat = Rays(rays.origins.reshape(-1, 3), None, rays.viewdirs.reshape(-1, 3), None)
    whole = paths.summarize(*paths.march(model, variables, flat))
    assert 100 < int((whole["nodes"] > 0).sum()) < 40 * 48 - 100                 # the crop holds both kinds of ray
    for chunk in (512, 700, 8192):                                               # 1920 rays: 3 full + 1 ragged chunk, 2 + 1 ragged, one chunk
        maps = paths.view_maps(model, variables, rays, chunk=chunk)
        assert sorted(maps) == ["bend", "first", "last", "nodes", "optical", "refracted"]
        for k, v in whole.items():
            assert tuple(maps[k].shape) == (40, 48) and maps[k].dtype == v.dtype and torch.equal(maps[k].reshape(-1), v), (chunk, k)
        assert maps["refracted"].dtype == torch.bool and torch.equal(maps["refracted"], maps["nodes"] > 0)
    vis = paths.visualize_maps(maps)
    assert sorted(vis) == ["bend", "mask", "optical"] and tuple(vis["mask"].shape) == (40, 48) and tuple(vis["bend"].shape) == (40, 48, 3)
    assert set(np.unique(vis["mask"].cpu().numpy()).tolist()) == {0.0, 1.0}
    for k in ("bend", "optical"):
        assert bool(torch.isfinite(vis[k]).all())
        assert bool((vis[k][~maps["refracted"]] == 1).all())                     # white where the ray does not refract
    none = dict(maps, refracted=torch.zeros_like(maps["refracted"]))             # a view no ray refracts in: white, never NaN
    for k, v in paths.visualize_maps(none).items():
        assert bool((v == (0 if k == "mask" else 1)).all()), k


def test_trace_pixels_gives_the_taps_of_forward(crop):
    from samplenerfro_amd import paths, prng
    from samplenerfro_amd.utils import Rays
    model, variables, rays = crop["model"], crop["variables"], crop["rays"]
    rng = prng.PRNGKey(4)
    pixels = [(3, 5), (30, 40), (39, 47)]
    c2w = np.arange(12, dtype=F32).reshape(3, 4)
    recs = paths.trace_pixels(model, variables, rays, pixels, rng, transform=c2w)
    _, key_0, key_1 = prng.split(rng, 3)                                         # as utils.render_image hands them to the model
    taps = {}
    model.forward(variables, key_0, key_1, Rays(rays.origins.reshape(-1, 3), None, rays.viewdirs.reshape(-1, 3), None), False, taps=taps)
    N, Nc = model.num_samples, model.num_coarse_samples
    assert len(recs) == 3
    for (row, col), rec in zip(pixels, recs):
        r = row * 48 + col
        assert list(rec) == ["ray_pos", "ray_dir", "idx_grad", "transform", "ray_pos_c"] and rec["transform"] is c2w
        assert rec["ray_pos"].shape == (1, N, 3) and rec["ray_pos_c"].shape == (1, Nc, 3) and rec["ray_pos"].dtype == F32
        pos = taps["path_pd"][:, r, :3].cpu().numpy()
        assert np.array_equal(bits(rec["ray_pos"][0]), bits(pos))
        assert np.array_equal(bits(rec["ray_dir"][0]), bits(taps["path_dr"][:, r, :3]))
        assert np.array_equal(bits(rec["idx_grad"][0]), bits(taps["path_ior"][:, r, 1:4]))
        assert np.array_equal(bits(rec["ray_pos_c"][0]), bits(pos[np.asarray(taps["jitter"])]))
    with pytest.raises(ValueError):
        paths.trace_pixels(model, variables, rays, [(40, 0)], rng)
