"""Connected components without a GPU: the numpy helper against scipy, the argument errors of rnerf_components_* through the C ABI, and
the ValueErrors of the Python layer (raised before anything is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import components_cases as cases      # noqa: E402
import components_ref as ref          # noqa: E402


def scipy_labels(on, connectivity):
    """scipy.ndimage.label relabelled to the minimum linear index of each component."""
    ndi = pytest.importorskip("scipy.ndimage")
    lab, k = ndi.label(on, structure=ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))
    flat = lab.reshape(-1)
    first = np.full(k + 1, -1, np.int64)
    idx = np.nonzero(flat)[0]
    first[flat[idx][::-1]] = idx[::-1]          # the last write per label is its smallest index
    return first[flat].astype(np.int32).reshape(on.shape)


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_helper_equals_scipy(connectivity):
    pytest.importorskip("scipy.ndimage")
    for name, g in cases.small_cases().items():
        for phase in (1, 0):
            on = (g != 0) == bool(phase)
            assert np.array_equal(ref.label(g, connectivity, phase), scipy_labels(on, connectivity)), (name, phase)


def test_helper_on_the_closed_form_cases():
    cb = cases.checkerboard(9)
    assert len(ref.stats(ref.label(cb, 6))[0]) == 365
    assert len(ref.stats(ref.label(cb, 18))[0]) == 1 and len(ref.stats(ref.label(cb, 26))[0]) == 1
    g, length = cases.snake()
    roots, sizes, _ = ref.stats(ref.label(g, 6))
    assert length == 1427 and list(sizes) == [1427]
    corner, edge = cases.pair_lattice(34, (1, 1, 1)), cases.pair_lattice(34, (1, 1, 0))
    n = 11 ** 3
    assert [len(ref.stats(ref.label(corner, c))[0]) for c in (6, 18, 26)] == [2 * n, 2 * n, n]
    assert [len(ref.stats(ref.label(edge, c))[0]) for c in (6, 18, 26)] == [2 * n, n, n]
    # ranking: the lower root of two equal-sized components first
    two = np.zeros((6, 6, 12), np.uint8); two[3:5, 3:5, 8:10] = 1; two[0:2, 0:2, 0:2] = 1
    roots, sizes, border = ref.stats(ref.label(two, 6))
    assert list(sizes) == [8, 8] and roots[0] == 0 and roots[1] == (3 * 6 + 3) * 12 + 8 and list(border) == [True, False]


def test_helper_select_and_fill():
    g, shell, cavity = cases.shell_scene()
    mask, dropped, filled = ref.select(g, keep=1)
    assert np.array_equal(mask, shell) and int(dropped.sum()) == 24 and not filled.any()
    mask, _, filled = ref.select(g, keep=1, fill_holes=True)
    assert np.array_equal(mask, shell | cavity) and np.array_equal(filled, cavity)
    t = cases.torus()
    assert np.array_equal(ref.select(t, keep=1, fill_holes=True)[0], t != 0)
    closed = cases.box_with_cavity(None)
    assert int(ref.select(closed, fill_holes=True)[2].sum()) == 27
    for channel in ("straight", "diagonal"):
        assert not ref.select(cases.box_with_cavity(channel), connectivity=6, fill_holes=True)[2].any()
    # the diagonal channel is closed for a 6-connected empty phase (solid 26): the cavity, the channel voxel on its face and the isolated
    # middle one are filled; the third touches the outside through a face and stays open
    assert int(ref.select(cases.box_with_cavity("diagonal"), connectivity=26, fill_holes=True)[2].sum()) == 27 + 2


DIMS = ctypes.c_int32 * 3
P = ctypes.c_void_p


def test_argument_errors_need_no_device(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    ok = DIMS(4, 5, 6)
    assert lib.rnerf_components_workspace_bytes(ctypes.byref(ok)) >= 4
    bad_dims = [DIMS(0, 5, 6), DIMS(4, -1, 6), DIMS(2048, 1024, 1024), DIMS(1 << 30, 2, 1), DIMS(46341, 46341, 1)]
    for d in bad_dims:
        assert lib.rnerf_components_workspace_bytes(ctypes.byref(d)) == 0 and b"dims" in lib.rnerf_last_error()
    assert lib.rnerf_components_workspace_bytes(ctypes.byref(DIMS(2147483647, 1, 1))) >= 4          # 2^31 - 1 voxels is legal
    a, b, c = P(256), P(512), P(1024)                                                                 # never dereferenced
    # label
    assert lib.rnerf_components_label(None, ctypes.byref(ok), 1, 6, b, c, None) == -1 and b"null" in lib.rnerf_last_error()
    assert lib.rnerf_components_label(a, ctypes.byref(ok), 1, 6, None, c, None) == -1
    assert lib.rnerf_components_label(a, ctypes.byref(ok), 1, 6, b, None, None) == -1
    assert lib.rnerf_components_label(a, ctypes.byref(ok), 1, 7, b, c, None) == -1 and b"connectivity" in lib.rnerf_last_error()
    assert lib.rnerf_components_label(a, ctypes.byref(ok), 2, 6, b, c, None) == -1 and b"phase" in lib.rnerf_last_error()
    for d in bad_dims:
        assert lib.rnerf_components_label(a, ctypes.byref(d), 1, 6, b, c, None) == -1 and b"dims" in lib.rnerf_last_error()
    # stats
    assert lib.rnerf_components_stats(None, ctypes.byref(ok), a, b, c, None) == -1 and b"null" in lib.rnerf_last_error()
    assert lib.rnerf_components_stats(a, ctypes.byref(ok), None, b, c, None) == -1
    assert lib.rnerf_components_stats(a, ctypes.byref(ok), b, None, c, None) == -1
    assert lib.rnerf_components_stats(a, ctypes.byref(ok), b, c, None, None) == -1
    for d in bad_dims:
        assert lib.rnerf_components_stats(a, ctypes.byref(d), a, b, c, None) == -1 and b"dims" in lib.rnerf_last_error()
    # apply
    assert lib.rnerf_components_apply(a, b, 0.0, None, None, 0.0, None, 0, ctypes.byref(ok), None) == -1 and b"null" in lib.rnerf_last_error()
    assert lib.rnerf_components_apply(None, None, 0.0, None, None, 0.0, c, 0, ctypes.byref(ok), None) == -1 and b"pairs" in lib.rnerf_last_error()
    assert lib.rnerf_components_apply(a, None, 0.0, None, None, 0.0, c, 0, ctypes.byref(ok), None) == -1
    assert lib.rnerf_components_apply(a, b, 0.0, a, None, 0.0, c, 0, ctypes.byref(ok), None) == -1
    assert lib.rnerf_components_apply(a, b, 0.0, None, None, 0.0, c, 3, ctypes.byref(ok), None) == -1 and b"dtype" in lib.rnerf_last_error()
    for d in bad_dims:
        assert lib.rnerf_components_apply(a, b, 0.0, None, None, 0.0, c, 0, ctypes.byref(d), None) == -1 and b"dims" in lib.rnerf_last_error()


def test_python_layer_raises_before_anything_is_launched():
    pytest.importorskip("torch")
    from samplenerfro_amd import components, extract, visual_hull, voxelize
    g = np.zeros((4, 4, 4), np.uint8)
    for kw in (dict(keep=0), dict(keep=-3), dict(min_voxels=0), dict(connectivity=7), dict(connectivity=4)):
        with pytest.raises(ValueError):
            components.select(g, **kw)
        with pytest.raises(ValueError):
            visual_hull.clean(g.astype(np.int32), 10, **kw)
        with pytest.raises(ValueError):
            voxelize.clean(g.astype(np.float32), **kw)
        with pytest.raises(ValueError):
            extract.extract_mesh(None, None, **kw)
    with pytest.raises(ValueError):
        components.label(g, connectivity=8)
    with pytest.raises(ValueError):
        components.label(g, phase=2)
    with pytest.raises(ValueError, match="threshold"):
        visual_hull.clean(g.astype(np.int32), 10, threshold=1.0, fill_holes=True)
