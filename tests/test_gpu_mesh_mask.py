"""rnerf_mesh_depth / rnerf_mask_dilate on the device against tests/helpers/mesh_raster_ref.py (numpy float64, pinned by
tests/test_mesh_mask_host.py) and, for the example scene, against Blender's depth pass.

Both sides evaluate the expressions of include/rnerf.h in float64 with every operation rounded, so tri, hits and the float32 depth are
compared for equality: 0 pixels differ in any case below, no ulp of slack is used."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mesh_raster_ref as MR                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device_render(v, f, H, W, cam, znear=0.1, zfar=100.0, allow_skipped=False, with_skipped=False):
    """mesh_mask.render_depth from the helper's camera dict -> numpy (depth, tri, hits[, skipped])."""
    from samplenerfro_amd import mesh_mask as MM
    kw = dict(focal=cam["fx"]) if not cam["opencv"] else dict(cam_mat=[[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]])
    vv, ff = MM.upload_mesh(v, f, DEV)
    camera = MM._camera(H, W, kw.get("focal"), kw.get("cam_mat"), cam["pc"] == 0.5)
    d, t, h, s = MM._render_uploaded(vv, ff, cam["c2w"], H, W, camera, znear, zfar, True, True, allow_skipped)
    out = (d.cpu().numpy(), t.cpu().numpy(), h.cpu().numpy())
    return out + (int(s.cpu()),) if with_skipped else out


def assert_equal_to_helper(v, f, H, W, cam, **kw):
    got = device_render(v, f, H, W, cam, allow_skipped=True, with_skipped=True, **kw)
    want = MR.render(v, f, H, W, **cam, **kw)
    for name, g, w in zip(("depth", "tri", "hits"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{name}: {int((g != w).sum())} of {g.size} pixels differ"
    assert got[3] == want[3]
    return got


@pytest.mark.parametrize("mesh", ["icosphere", "tetrahedron"])
@pytest.mark.parametrize("H,W", [(70, 45), (45, 70)])
def test_small_meshes_equal_the_helper(mesh, H, W):
    """Sizes that are no multiple of the 16-pixel tile; both camera models, the OpenCV one with an off-centre principal point and
    fx != fy; pixel_center on and off.  Equality of tri, hits and the float32 depth: 0 pixels differ."""
    v, f = MR.icosphere(1) if mesh == "icosphere" else MR.tetrahedron()
    covered = 0
    for name, cam in MR.sphere_cameras(H, W).items():
        for pc in (0.5, 0.0):
            d, t, h, _ = assert_equal_to_helper(v, f, H, W, dict(cam, pc=pc))
            assert np.all(h[d > 0] == 2) and np.all(h[d == 0] == 0) and np.all((t >= 0) == (d > 0))      # closed and convex
            covered += int((d > 0).sum())
    assert covered > 0.2 * 4 * H * W


@pytest.mark.parametrize("blender", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_fill_rule_on_exact_integer_cases(reverse, blender):
    """The cases of tests/test_mesh_mask_host.py: a quad split along a diagonal through pixel centres, a fan around a vertex on one."""
    render = lambda v, f, H, W, cam: device_render(v, f, H, W, cam, znear=1.0, zfar=100.0, with_skipped=True)
    MR.check_planar(lambda name: MR.planar_run(render, name, reverse, blender))


def plane_cam(W=64, H=64, focal=64.0):
    """An OpenCV camera at the identity pose: (x, y, z) projects to (x focal / z + W / 2, y focal / z + H / 2)."""
    return MR.camera(MR.EYE4, cam_mat=[[focal, 0, W * 0.5], [0, focal, H * 0.5], [0, 0, 1]])


def test_bins_one_triangle_covering_the_whole_image():
    H = W = 64
    v = np.array([[-200.0, -100.0, 64.0], [200.0, -100.0, 64.0], [0.0, 300.0, 64.0]])
    d, t, h = assert_equal_to_helper(v, np.array([[0, 1, 2]], np.int32), H, W, plane_cam())[:3]
    assert np.all(d == 64.0) and np.all(t == 0) and np.all(h == 1)


def test_bins_a_thousand_triangles_stacked_in_one_tile():
    """More than one LDS batch (128 faces) in one tile's list; the nearest of 1000 depths wins whatever the order of the list."""
    H = W = 64
    rng = np.random.default_rng(11)
    z = rng.permutation(1000) * 0.01 + 5.0
    base = np.array([[2.0, 2.0], [13.0, 3.0], [4.0, 14.0]]) + 16.0 - 32.0               # inside tile (1, 1), in pixels from the centre
    v = np.concatenate([np.concatenate([base * (zz / 64.0), np.full((3, 1), zz)], 1) for zz in z])
    f = np.arange(3000, dtype=np.int32).reshape(1000, 3)
    d, t, h = assert_equal_to_helper(v, f, H, W, plane_cam())[:3]
    assert h.max() == 1000 and d[h == 1000].min() == np.float32(5.0) and np.all(t[h == 1000] == int(np.argmin(z)))
    assert np.all(h[:16] == 0) and np.all(h[32:] == 0) and np.all(h[:, :16] == 0) and np.all(h[:, 32:] == 0)


def test_bins_off_image_behind_near_far_and_degenerate():
    H, W = 40, 56
    cam = plane_cam(W, H)
    tri = lambda x0, y0, x1, y1, x2, y2, z: [[x0 * z / 64.0, y0 * z / 64.0, z], [x1 * z / 64.0, y1 * z / 64.0, z], [x2 * z / 64.0, y2 * z / 64.0, z]]
    v = np.array(tri(-60, -40, 70, -10, -5, 60, 8.0)                 # 0: partly off every side of the image
                 + tri(100, 100, 140, 100, 100, 150, 8.0)            # 1: wholly outside
                 + [[0.0, 0.0, -1.0], [1.0, 0.0, 4.0], [0.0, 1.0, 4.0]]   # 2: one vertex behind the camera
                 + tri(-20, -15, -10, -15, -20, -5, 0.05)            # 3: in front of znear
                 + tri(5, 5, 20, 5, 5, 15, 200.0)                    # 4: beyond zfar
                 + tri(-25, 10, -15, 12, -5, 14, 6.0)                # 5: zero area (collinear)
                 + tri(-20, -15, -10, -15, -20, -5, 3.0))            # 6: a second kept face under face 3's footprint
    f = np.arange(21, dtype=np.int32).reshape(7, 3)
    d, t, h, skipped = assert_equal_to_helper(v, f, H, W, cam)
    assert skipped == 1 and set(np.unique(t)) == {-1, 0, 6}
    for edge in (d[0], d[-1], d[:, 0], d[:, -1]):
        assert (edge == 8.0).any()                                                    # face 0 reaches every side
    without = np.delete(np.arange(7), 2)
    d2, t2, h2, skipped2 = assert_equal_to_helper(v, f[without], H, W, cam)
    assert skipped2 == 0 and np.array_equal(d, d2) and np.array_equal(h, h2)          # the skipped face left the rest unchanged
    from samplenerfro_amd import _lib, mesh_mask as MM
    with pytest.raises(_lib.RnerfError, match="behind the camera plane"):
        MM.render_depth(v, f, cam["c2w"], H, W, cam_mat=[[64.0, 0, W * 0.5], [0, 64.0, H * 0.5], [0, 0, 1]])
    with pytest.raises(ValueError, match="index vertices"):
        MM.render_depth(v, f + 1, cam["c2w"], H, W, cam_mat=[[64.0, 0, W * 0.5], [0, 64.0, H * 0.5], [0, 0, 1]])


def test_bins_no_faces_and_a_one_pixel_image():
    from samplenerfro_amd import mesh_mask as MM
    cam = plane_cam(5, 3)
    d, t, h = MM.render_depth(np.zeros((0, 3)), np.zeros((0, 3), np.int32), cam["c2w"], 3, 5, cam_mat=[[64.0, 0, 2.5], [0, 64.0, 1.5], [0, 0, 1]],
                              return_tri=True, return_hits=True)
    assert d.shape == (3, 5) and torch.all(d == 0) and torch.all(t == -1) and torch.all(h == 0)
    v = np.array([[-1.0, -1.0, 2.0], [3.0, -1.0, 2.0], [-1.0, 3.0, 2.0]])
    f = np.array([[0, 1, 2]], np.int32)
    d, t, h = assert_equal_to_helper(v, f, 1, 1, plane_cam(1, 1))[:3]
    assert d.shape == (1, 1) and d[0, 0] == 2.0 and t[0, 0] == 0 and h[0, 0] == 1
    d, t, h = assert_equal_to_helper(v + [10.0, 0.0, 0.0], f, 1, 1, plane_cam(1, 1))[:3]
    assert d[0, 0] == 0.0 and t[0, 0] == -1 and h[0, 0] == 0


def test_face_order_and_repeatability():
    H, W = 70, 45
    v, f = MR.icosphere(1)
    cam = MR.sphere_cameras(H, W)["opencv"]
    d, t, h = device_render(v, f, H, W, cam)
    perm = np.random.default_rng(3).permutation(len(f))
    d2, t2, h2 = device_render(v, f[perm], H, W, cam)
    assert np.array_equal(d, d2) and np.array_equal(h, h2)
    assert np.array_equal(np.where(t2 >= 0, perm[np.maximum(t2, 0)], -1), t)          # tri maps through the permutation
    d3, t3, h3 = device_render(v, f, H, W, cam)
    assert d.tobytes() == d3.tobytes() and t.tobytes() == t3.tobytes() and h.tobytes() == h3.tobytes()


@pytest.fixture(scope="module")
def example():
    """The example OBJ from the example camera at 800 x 800: one render, and its dilated mask."""
    import cases
    from samplenerfro_amd import mesh_mask as MM
    verts, faces, _ = cases.load_example_obj()
    H, W, focal, _ = MR.example_camera()
    v, f = MM.upload_mesh(cases.example_obj_world(verts), faces, DEV)
    depth, hits = MM.render_depth(v, f, cases.EXAMPLE_C2W, H, W, focal=focal, return_hits=True)
    mask = MM.render_mask(v, f, cases.EXAMPLE_C2W, H, W, focal=focal, dilate=35)
    return dict(depth=depth, hits=hits, mask=mask)


def test_example_scene_against_blenders_depth_pass(example):
    MR.check_example(example["depth"].cpu().numpy(), example["hits"].cpu().numpy())


def test_example_mask_contains_blenders_surface_and_its_bounding_rectangle(example):
    from samplenerfro_amd import mesh_mask as MM
    mask = example["mask"]
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (800, 800)
    m = mask.cpu().numpy()
    assert set(np.unique(m)) == {0, 255}
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_depth.npz"))
    surface = z["z"] < 1e9
    assert surface.sum() > 4000 and np.all(m[z["rows"]][:, z["cols"]][surface] == 255)
    assert np.array_equal(m, MR.dilate(example["depth"].cpu().numpy() != 0, 35, 35))
    assert MM.bounding_rect(mask) == MR.bounding_rect(m)
    assert np.array_equal(MM.dilate(example["depth"] != 0, 35).cpu().numpy(), m)      # the 800 x 800 silhouette through dilate()


def dilate_cases():
    corners = np.zeros((37, 50), np.uint8)
    for r, c in ((0, 0), (0, 49), (36, 0), (36, 49), (18, 25)):
        corners[r, c] = 7                                                             # any value > 0 is set
    rng = np.random.default_rng(2)
    return {"corners_37x50": (corners, 35), "corners_50x37": (np.ascontiguousarray(corners.T), 35),
            "identity": ((rng.random((21, 33)) < 0.3).astype(np.uint8), 1), "empty": (np.zeros((37, 50), np.uint8), 35),
            "full": (np.full((19, 23), 255, np.uint8), 35), "sparse_3": ((rng.random((40, 70)) < 0.01).astype(np.uint8) * 255, 3)}


@pytest.mark.parametrize("name", sorted(dilate_cases()))
def test_dilate_against_the_helper(name):
    from samplenerfro_amd import mesh_mask as MM
    ndi = pytest.importorskip("scipy.ndimage")
    m, size = dilate_cases()[name]
    want = MR.dilate(m, size, size)
    assert np.array_equal(want, ndi.maximum_filter((m > 0).astype(np.uint8) * 255, size=(size, size), mode="constant", cval=0))
    got = MM.dilate(torch.from_numpy(m).to(DEV), size)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert MM.bounding_rect(got) == MR.bounding_rect(want)
    if name == "empty":
        assert MM.bounding_rect(got) == (0, 0, 0, 0)
    if name == "identity":
        assert np.array_equal(got.cpu().numpy(), (m > 0) * 255)


def test_dilate_3x5_through_the_c_entry_point():
    from samplenerfro_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(8)
    m = (rng.random((50, 37)) < 0.02).astype(np.uint8)
    H, W = m.shape
    md = torch.from_numpy(m).to(DEV)
    out = torch.empty_like(md)
    bbox = torch.empty(4, dtype=torch.int32, device=DEV)
    ws = torch.empty((lib.rnerf_mask_dilate_workspace_bytes(H, W) + 7) // 8, dtype=torch.int64, device=DEV)
    _lib.check(lib.rnerf_mask_dilate(_lib.ptr(md), H, W, 3, 5, _lib.ptr(out), _lib.ptr(bbox), _lib.ptr(ws), _lib.current_stream()), "rnerf_mask_dilate")
    want = MR.dilate(m, 3, 5)
    assert not np.array_equal(want, MR.dilate(m, 5, 3))                               # ky and kx are told apart
    assert np.array_equal(out.cpu().numpy(), want) and tuple(int(x) for x in bbox.cpu()) == MR.bounding_rect(want)


def test_render_masks_uploads_once_and_matches_render_mask(tmp_path):
    from samplenerfro_amd import mesh_mask as MM
    H, W = 45, 70
    v, f = MR.icosphere(1)
    cams = MR.sphere_cameras(H, W)
    c2ws = [cams["blender"]["c2w"], MR.look_at((-2.0, 2.0, 0.5))]
    masks = list(MM.render_masks(v, f, c2ws, H, W, focal=cams["blender"]["fx"], dilate=5))
    assert len(masks) == 2 and not torch.equal(masks[0], masks[1])
    for c2w, m in zip(c2ws, masks):
        assert torch.equal(m, MM.render_mask(v, f, c2w, H, W, focal=cams["blender"]["fx"], dilate=5))
        bare = MM.render_mask(v, f, c2w, H, W, focal=cams["blender"]["fx"], dilate=0)
        want, _, _, _ = MR.render(v, f, H, W, **MR.camera(c2w, focal=cams["blender"]["fx"], H=H, W=W))
        assert np.array_equal(bare.cpu().numpy(), (want != 0) * 255) and np.array_equal(m.cpu().numpy(), MR.dilate(want != 0, 5, 5))
    MM.save_mask(str(tmp_path / "mask_r_0.png"), masks[0])
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "mask_r_0.png")), masks[0].cpu().numpy())
