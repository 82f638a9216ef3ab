"""The plumbing the evaluation modules share (ops.workspace, ops.device_of, ops.as_f32): the kept workspaces of ops.flip / ops.lpips, the
uploads of numpy arrays and CPU tensors, and the error of a workspace query that answers 0.  Everything here is compared bit for bit;
no image is larger than 64 x 64 x 3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lpips_ref as R               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def images(seed, *shape):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(0, 1, shape).astype(np.float32)


def kept(query, stream):
    """The buffers ops.workspace keeps for `query` on device 0 and `stream`."""
    from samplenerfro_amd import ops
    return [ws for (name, index, handle), ws in ops._workspaces.items() if (name, index, handle) == (query, 0, stream.cuda_stream)]


def flip_exact(a, b, ppd):
    """rnerf_flip's mean through the library itself, with a workspace of exactly the bytes it asks for."""
    from samplenerfro_amd import _lib
    lib = _lib.load()
    H, W = int(a.shape[0]), int(a.shape[1])
    nb = lib.rnerf_flip_workspace_bytes(1, H, W, ppd)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    mean = torch.empty((), dtype=torch.float32, device=DEV)
    _lib.check(lib.rnerf_flip(a.data_ptr(), b.data_ptr(), 1, H, W, ppd, None, mean.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "rnerf_flip")
    return mean, nb


def lpips_exact(a, b, weights):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    H, W = int(a.shape[0]), int(a.shape[1])
    nb = lib.rnerf_lpips_workspace_bytes(1, H, W)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    value = torch.empty((), dtype=torch.float32, device=DEV)
    _lib.check(lib.rnerf_lpips(a.data_ptr(), b.data_ptr(), 1, H, W, weights.flat.data_ptr(), None, value.data_ptr(), None, ws.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "rnerf_lpips")
    return value, nb


def check_kept_workspace(query, call, exact, small, large):
    """call(a, b) is the wrapper that keeps its workspace, exact(a, b) -> (result, bytes) the same entry point with a fresh workspace of
    exactly its size; small / large are image pairs on the device."""
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    assert kept(query, s1) == [] and kept(query, s2) == []
    with torch.cuda.stream(s1):
        first, again = call(*small), call(*small)
        assert torch.equal(first.cpu(), again.cpu())
        (ws_small,) = kept(query, s1)                                   # exactly one buffer for this device and stream
        want_small, nb_small = exact(*small)
        assert ws_small.dtype == torch.uint8 and ws_small.numel() == nb_small
        assert torch.equal(first.cpu(), want_small.cpu())
        big = call(*large)
        (ws_large,) = kept(query, s1)                                   # a larger shape replaces it with a larger one
        want_large, nb_large = exact(*large)
        assert nb_large > nb_small and ws_large.numel() == nb_large and ws_large.data_ptr() != ws_small.data_ptr()
        assert torch.equal(big.cpu(), want_large.cpu())
        after = call(*small)                                            # a smaller shape afterwards reuses the larger one
        (ws_after,) = kept(query, s1)
        assert ws_after.data_ptr() == ws_large.data_ptr() and ws_after.numel() == nb_large
        assert torch.equal(after.cpu(), want_small.cpu())
    with torch.cuda.stream(s2):                                          # a second stream gets its own buffer
        other = call(*small)
        (ws_other,) = kept(query, s2)
        assert ws_other.data_ptr() != ws_large.data_ptr() and ws_other.numel() == nb_small
        assert torch.equal(other.cpu(), want_small.cpu())
    assert len(kept(query, s1)) == 1


def test_flip_keeps_one_workspace_per_device_and_stream():
    from samplenerfro_amd import ops, utils
    ppd = utils.FLIP_PPD_SUMMARY
    small, large = [T(x) for x in images(1, 24, 40, 3)], [T(x) for x in images(2, 48, 64, 3)]
    check_kept_workspace("rnerf_flip_workspace_bytes", lambda a, b: ops.flip(a, b, pixels_per_degree=ppd), lambda a, b: flip_exact(a, b, ppd),
                         small, large)


def test_lpips_keeps_one_workspace_per_device_and_stream():
    from samplenerfro_amd import lpips, ops
    w = R.weight_set()
    weights = lpips.from_tensors(w["convs"], w["biases"], w["lins"], device=DEV)
    small, large = [T(x) for x in images(3, 40, 40, 3)], [T(x) for x in images(4, 48, 64, 3)]
    check_kept_workspace("rnerf_lpips_workspace_bytes", lambda a, b: ops.lpips(a, b, weights), lambda a, b: lpips_exact(a, b, weights), small,
                         large)


def test_only_flip_and_lpips_keep_a_workspace():
    from samplenerfro_amd import errmap, ops, vis
    a, b = images(5, 33, 47, 3)
    errmap.error_maps(T(a), T(b))
    vis.visualize_suite(T(a[..., 0] + 0.5), T(b[..., 0]))
    ops.ssim(T(a), T(b), max_val=1.0)
    assert {name for name, _, _ in ops._workspaces} <= {"rnerf_flip_workspace_bytes", "rnerf_lpips_workspace_bytes"}


def same_bits(x, y):
    if isinstance(x, dict):
        return sorted(x) == sorted(y) and all(same_bits(x[k], y[k]) for k in x)
    return x.is_cuda and y.is_cuda and x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_uploads_give_the_bits_of_device_inputs():
    """(numpy, numpy), (CPU tensor, device tensor) and (device, device) inputs give the same bits."""
    from samplenerfro_amd import errmap, lpips, mesh_mask, utils, vis
    a, b = images(6, 40, 40, 3)
    w = R.weight_set()
    weights = lpips.from_tensors(w["convs"], w["biases"], w["lins"], device=DEV)
    depth, acc = (1.0 + 4.0 * a[..., 0]).astype(np.float32), b[..., 0]
    pairs = {"compute_ssim": (lambda x, y: utils.compute_ssim(x, y, 1.0), a, b),
             "compute_ssim map": (lambda x, y: utils.compute_ssim(x, y, 1.0, return_map=True), a, b),
             "compute_flip": (lambda x, y: utils.compute_flip(x, y, utils.FLIP_PPD_SUMMARY), a, b),
             "compute_lpips": (lambda x, y: utils.compute_lpips(x, y, weights), a, b),
             "error_maps": (lambda x, y: errmap.error_maps(x, y), a, b),
             "error_maps lpips": (lambda x, y: errmap.error_maps(x, y, lpips=weights), a, b),
             "visualize_depth": (lambda x, y: vis.visualize_depth(x, y), depth, acc),
             "visualize_normals": (lambda x, y: vis.visualize_normals(x, y), depth, acc)}
    for name, (fn, x, y) in pairs.items():
        want = fn(T(x), T(y))
        assert same_bits(fn(x, y), want), f"{name}: numpy inputs"
        assert same_bits(fn(torch.from_numpy(x), T(y)), want), f"{name}: a CPU tensor beside a device tensor"
        assert same_bits(fn(x.astype(np.float64), y.astype(np.float64)), want), f"{name}: float64 numpy inputs become float32"
    mask = (a[..., 0] > 0.97).astype(np.uint8)
    want = mesh_mask.dilate(T(mask), 5)
    assert want.dtype == torch.uint8 and 0 < int((want == 255).sum()) < want.numel()
    assert same_bits(mesh_mask.dilate(mask, 5), want) and same_bits(mesh_mask.dilate(torch.from_numpy(mask), 5), want)
    assert same_bits(mesh_mask.dilate(mask.astype(bool), 5), want)


def test_a_workspace_query_that_answers_zero_raises_the_library_error():
    from samplenerfro_amd import _lib, components, vis
    depth = T(images(7, 12, 16)[0] + 1.0)
    with pytest.raises(_lib.RnerfError, match=r"rnerf_vis_depth_workspace_bytes failed \(-1\): rnerf_vis_depth: ignore_frac must be in \[0, 0\.5\)"):
        vis.visualize_depth(depth, ignore_frac=0.5)
    for grid in (np.zeros((0, 4, 4), np.uint8), torch.zeros((0, 4, 4), dtype=torch.uint8, device=DEV)):
        with pytest.raises(_lib.RnerfError, match=r"rnerf_components_workspace_bytes failed \(-1\): rnerf_components_workspace_bytes: need dims\[0\.\.2\] >= 1"):
            components.label(grid)
    lib = _lib.load()
    assert lib.rnerf_components_workspace_bytes(C.byref((C.c_int32 * 3)(4, 4, 4))) > 0
