"""Mesh silhouettes and masked evaluation without a GPU.

- tests/helpers/mesh_raster_ref.py (the numpy float64 restatement of rnerf_mesh_depth the device tests compare against) is itself pinned:
  against an independent brute-force Moeller-Trumbore cast, on exact-integer fill-rule cases, and against ground truth this repository
  did not make — Blender's depth pass of the example view (tests/golden/example_depth.npz) over the reference's own marching-cubes OBJ
  (tests/golden/example_obj.npz).  The bars of the example scene are those of a float64 ray cast of that OBJ (silhouette agreement
  0.9967; planar depth error median -0.189, 95th percentile 0.344, maximum 1.17 voxel pitches; every ray meets the mesh an even
  number of times), with room for the tie rule and nothing else: the data is fixed.
- the dilation / bounding-rectangle helpers against scipy, the file-name and suffix rules of the reference's scripts;
- the C ABI: the new symbols are declared, bound and exported, and every argument error is reported without a device."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import mesh_raster_ref as MR                 # noqa: E402

NEW_SYMBOLS = ("rnerf_mesh_depth_workspace_bytes", "rnerf_mesh_depth", "rnerf_mask_dilate_workspace_bytes", "rnerf_mask_dilate")
EYE4 = MR.EYE4


@pytest.mark.parametrize("model", ["blender", "opencv"])
def test_helper_agrees_with_the_brute_force_cast(model):
    H, W = 48, 64
    v, f = MR.icosphere(1)
    assert f.shape == (80, 3)
    cam = MR.sphere_cameras(H, W)[model]
    depth, tri, hits, skipped = MR.render(v, f, H, W, depth64=True, **cam)
    bdepth, bhits = MR.cast(v, f, H, W, **cam)
    assert skipped == 0 and 0.2 < (depth > 0).mean() < 0.9
    differ = np.nonzero((depth > 0) != (bdepth > 0))
    near = MR.edge_distance(v, f, differ[0], differ[1], **cam) if len(differ[0]) else np.zeros(0)
    print(f"{model}: {int((depth > 0).sum())} covered pixels, {len(differ[0])} differ from the cast (all within 1e-9 px of an edge)")
    assert np.all(near <= 1e-9)
    both = (depth > 0) & (bdepth > 0)
    assert np.all(np.abs(depth[both] - bdepth[both]) <= 1e-12 * bdepth[both])
    assert np.all(hits[depth > 0] == 2) and np.all(tri[depth > 0] >= 0)       # a closed convex mesh, watertight rule: in and out, everywhere
    d32, _, _, _ = MR.render(v, f, H, W, **cam)
    assert d32.dtype == np.float32 and np.array_equal(d32, depth.astype(np.float32))


@pytest.mark.parametrize("blender", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_helper_fill_rule_on_exact_integer_cases(reverse, blender):
    render = lambda v, f, H, W, cam: MR.render(v, f, H, W, znear=1.0, zfar=100.0, **cam)
    MR.check_planar(lambda name: MR.planar_run(render, name, reverse, blender))


def test_helper_on_the_example_obj_against_blenders_depth_pass():
    import cases
    verts, faces, _ = cases.load_example_obj()
    H, W, _, cam = MR.example_camera()
    depth, _, hits, skipped = MR.render(cases.example_obj_world(verts), faces, H, W, **cam)
    assert skipped == 0
    MR.check_example(depth, hits)


def test_dilation_helper_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for (H, W), (ky, kx) in [((37, 50), (35, 35)), ((50, 37), (35, 35)), ((20, 31), (3, 5)), ((9, 9), (1, 1)), ((6, 4), (35, 35))]:
        m = (rng.random((H, W)) < 0.02).astype(np.uint8) * 255
        m[0, 0] = m[-1, -1] = 255
        want = ndi.maximum_filter(m, size=(ky, kx), mode="constant", cval=0)
        assert np.array_equal(MR.dilate(m, ky, kx), want)
    assert np.array_equal(MR.dilate(np.zeros((5, 7), np.uint8), 35, 35), np.zeros((5, 7), np.uint8))


def test_bounding_rect_rule():
    m = np.zeros((20, 30), np.uint8)
    assert MR.bounding_rect(m) == (0, 0, 0, 0)                                # cv2.boundingRect of an empty image
    m[4, 7] = 1
    assert MR.bounding_rect(m) == (7, 4, 1, 1)
    m[15, 2] = 255; m[9, 29] = 3
    assert MR.bounding_rect(m) == (2, 4, 28, 12)                              # smallest set column / row, extent to the largest inclusive


def test_mask_file_name_rule():
    from samplenerfro_amd import mesh_mask
    assert mesh_mask.mask_file_name("./test/r_12", "blender") == os.path.join("./test", "mask_r_12.png")
    assert mesh_mask.mask_file_name("imgs/IMG_0042.JPG", "opencv") == os.path.join("imgs", "mask_IMG_0042.png")
    assert mesh_mask.mask_file_name("r_0") == "mask_r_0.png"
    with pytest.raises(ValueError):
        mesh_mask.mask_file_name("r_0", "llff")


def test_suffix_rule():
    from samplenerfro_amd import evaluate
    for MASK, CROP, mode in [(False, False, None), (True, False, "mask"), (False, True, "crop"), (True, True, "mask_crop")]:
        want = "_mask" if MASK else "" + "_crop" if CROP else ""             # the expression of metric/summary.py:165, as Python parses it
        assert evaluate.mask_suffix(mode) == want
    assert evaluate.mask_suffix("mask_crop") == "_mask"                       # the quirk: not "_mask_crop"
    with pytest.raises(ValueError):
        evaluate.mask_suffix("both")


def test_save_mask_writes_a_single_channel_png(tmp_path):
    from PIL import Image
    from samplenerfro_amd import mesh_mask
    m = np.zeros((6, 9), np.uint8); m[2:4, 3:8] = 255
    mesh_mask.save_mask(str(tmp_path / "mask_r_0.png"), m)
    im = Image.open(tmp_path / "mask_r_0.png")
    assert im.mode == "L" and np.array_equal(np.asarray(im), m)


def test_new_symbols_are_declared_bound_and_exported(lib_path):
    from samplenerfro_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rnerf.h")).read()
    lib = ctypes.CDLL(lib_path)
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.load().rnerf_version() == 4                                  # appended: the ABI version does not move
    for site in ("render_mask.py:84-91", "render_mask.py:92-93", "summary.py:202"):
        assert site in hdr
    import samplenerfro_amd
    assert samplenerfro_amd.mesh_mask.render_masks is not None


def test_argument_errors_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p, mis = ctypes.c_void_p(256), ctypes.c_void_p(260)
    err = lambda: lib.rnerf_last_error()
    c2w = np.ascontiguousarray(EYE4).ctypes.data_as(ctypes.c_void_p)

    def depth(verts=p, V=10, faces=p, F=10, cam=c2w, opencv=1, fx=50.0, fy=50.0, cx=8.0, cy=8.0, pc=0.5, H=16, W=16, znear=0.1, zfar=10.0,
              out=p, tri=p, hits=p, skipped=p, ws=p):
        return lib.rnerf_mesh_depth(verts, V, faces, F, cam, opencv, fx, fy, cx, cy, pc, H, W, znear, zfar, out, tri, hits, skipped, ws, None)

    for kw in ({"cam": None}, {"out": None}, {"skipped": None}, {"verts": None}, {"faces": None}, {"ws": None}, {"V": 0}):
        assert depth(**kw) == -1 and b"null pointer" in err(), kw
    for kw in ({"V": -1}, {"V": 2 ** 31}, {"F": -1}, {"F": 2 ** 29}, {"H": 0}, {"W": 0}, {"H": -4}, {"H": 2 ** 16, "W": 2 ** 15}):
        assert depth(**kw) == -1 and b"height * width < 2^31" in err(), kw
    assert depth(opencv=2) == -1 and b"opencv must be 0 or 1" in err()
    for kw in ({"fx": 0.0}, {"fy": 0.0}, {"fx": math.inf}, {"fy": math.nan}, {"cx": math.nan}, {"cy": math.inf}, {"pc": math.nan}):
        assert depth(**kw) == -1 and b"finite" in err(), kw
    flat = np.zeros((3, 4), np.float32); flat[0, 0] = flat[1, 1] = 1.0       # a rank-2 "rotation"
    assert depth(cam=flat.ctypes.data_as(ctypes.c_void_p)) == -1 and b"no finite inverse" in err()
    for kw in ({"znear": 1.0, "zfar": 1.0}, {"znear": 2.0, "zfar": 1.0}, {"znear": math.nan}, {"zfar": math.nan}):
        assert depth(**kw) == -1 and b"znear < zfar" in err(), kw
    for kw in ({"verts": mis}, {"ws": mis}, {"skipped": mis}, {"ws": ctypes.c_void_p(264)}):
        assert depth(**kw) == -1 and b"aligned" in err(), kw
    # the workspace query: its parts (include/rnerf.h), and the same size limits
    up16 = lambda n: (n + 15) // 16 * 16
    V, F, H, W = 1001, 2003, 70, 45
    tiles = ((H + 15) // 16) * ((W + 15) // 16)
    want = up16(24 * V) + up16(16 * F) + up16(4 * (tiles + 1)) + up16(4 * tiles) + up16(16 * F) + 16 + up16(4 * F)
    assert lib.rnerf_mesh_depth_workspace_bytes(V, F, H, W) == want
    assert lib.rnerf_mesh_depth_workspace_bytes(0, 0, 1, 1) > 0
    for bad in ((-1, 1, 4, 4), (1, 2 ** 29, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, 2 ** 16, 2 ** 15)):
        assert lib.rnerf_mesh_depth_workspace_bytes(*bad) == 0 and b"height * width < 2^31" in err(), bad

    def dil(mask=p, H=16, W=16, ky=35, kx=35, out=ctypes.c_void_p(4096), bbox=p, ws=p):
        return lib.rnerf_mask_dilate(mask, H, W, ky, kx, out, bbox, ws, None)

    for kw in ({"mask": None}, {"out": None}, {"ws": None}):
        assert dil(**kw) == -1 and b"null pointer" in err(), kw
    for kw in ({"H": 0}, {"W": 0}, {"W": -1}, {"H": 2 ** 16, "W": 2 ** 15}):
        assert dil(**kw) == -1 and b"height * width < 2^31" in err(), kw
    for kw in ({"ky": 0}, {"kx": 0}, {"ky": 34}, {"kx": 2}, {"ky": -3}):
        assert dil(**kw) == -1 and b"odd" in err(), kw
    for out in (256, 256 + 255, 256 - 255):                                   # out overlapping mask anywhere
        assert dil(out=ctypes.c_void_p(out)) == -1 and b"alias" in err()
    assert dil(ws=mis) == -1 and b"aligned" in err()
    assert dil(bbox=ctypes.c_void_p(258)) == -1 and b"aligned" in err()
    assert lib.rnerf_mask_dilate_workspace_bytes(37, 50) == up16(37 * 50) + 16 * ((37 * 50 + 255) // 256)
    assert lib.rnerf_mask_dilate_workspace_bytes(0, 5) == 0 and b"height * width < 2^31" in err()
    assert lib.rnerf_mask_dilate_workspace_bytes(2 ** 16, 2 ** 15) == 0
