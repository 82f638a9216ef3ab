"""rnerf_lpips on the device against the float64 restatement of tests/helpers/lpips_ref.py, with seeded random weights.

Bound (that of tests/test_gpu_errmap.py and tests/test_gpu_flip.py): for the value, the map and each d_l separately,
|device - float64| <= max(4 e_ref, 1e-6), e_ref = the restatement's own float32 error against float64 on the same case.  No case is
excluded.  Every figure is printed before it is asserted.

Measured on an MI355X, the largest over the six cases: value |device - float64| 3.7e-8 (0.04 x the bound; 0.005 - 1.0 x e_ref), map 3.0e-7
(0.30 x the bound; 0.66 - 1.20 x e_ref), the d_l 1.6e-7 (0.16 x the bound; 0.20 - 2.19 x e_ref), the dead taps exactly 0.
"""
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


_weights = {}


def device_weights(conv3_bias=None):
    from samplenerfro_amd import lpips
    if conv3_bias not in _weights:
        w = R.weight_set(conv3_bias)
        _weights[conv3_bias] = lpips.from_tensors(w["convs"], w["biases"], w["lins"], device=DEV)
        assert torch.equal(_weights[conv3_bias].flat.cpu(), R.flat(w))
    return _weights[conv3_bias]


def run(name, a=None, b=None):
    """-> (map, value, [d_l]) as numpy arrays from one call of rnerf_lpips with every output."""
    from samplenerfro_amd import ops
    c = R.case(name)
    a = c["img0"] if a is None else a
    b = c["img1"] if b is None else b
    smap, value, layers = ops.lpips(T(a), T(b), device_weights(R.CASES[name][4]), return_both=True, return_layers=True)
    return smap.cpu().numpy(), value.cpu().numpy(), [d.cpu().numpy() for d in layers]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_value_map_and_every_layer_against_float64(name):
    c = R.case(name)
    v64, m64, l64 = c["ref64"]
    v32, m32, l32 = c["ref32"]
    smap, value, layers = run(name)
    assert smap.dtype == np.float32 and smap.shape == m64.shape and value.shape == v64.shape
    assert np.isfinite(smap).all() and np.isfinite(value).all()
    failures = []
    for what, got, want, ref32 in [("value", value, v64, v32), ("map", smap, m64, m32)] + [(f"d_{l}", layers[l], l64[l], l32[l]) for l in range(5)]:
        assert got.shape == want.shape, what
        e_ref = float(np.abs(ref32 - want).max())
        bound = max(4.0 * e_ref, 1e-6)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"lpips {name} {what}: |device - f64| {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}  max|want| {np.abs(want).max():.3e}")
        if not err <= bound:
            failures.append((what, err, bound))
    assert not failures, failures
    if name == "dead":                       # conv3's bias at -1e3: taps 2-4 are all zero, 0 / (0 + 1e-10) = 0
        assert all(np.all(d == 0) for d in layers[2:]) and layers[0].max() > 0 and layers[1].max() > 0


def test_identical_images_give_exactly_zero():
    for name in ("67x93", "batch2"):
        c = R.case(name)
        smap, value, layers = run(name, c["img1"], c["img1"])
        assert np.all(value == 0) and np.all(smap == 0) and all(np.all(d == 0) for d in layers), name


def test_swapped_arguments_and_a_second_call_give_the_same_bytes():
    for name in ("67x93", "batch2", "const"):
        c = R.case(name)
        first, again, swapped = run(name), run(name), run(name, c["img1"], c["img0"])
        for other in (again, swapped):
            assert first[0].tobytes() == other[0].tobytes() and first[1].tobytes() == other[1].tobytes(), name
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first[2], other[2])), name


def test_each_output_alone_gives_the_bytes_of_the_full_call():
    """Straight through the C ABI: map with value null, value with map null, layer_maps alone."""
    from samplenerfro_amd import _lib, ops
    lib = _lib.load()
    name = "batch2"
    c = R.case(name)
    n, H, W = c["img0"].shape[:3]
    a, b, w = T(c["img0"]), T(c["img1"]), device_weights().flat
    smap, value, layers = run(name)
    ws = torch.empty(lib.rnerf_lpips_workspace_bytes(n, H, W), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    total = sum(h * w_ for h, w_ in ops.lpips_layer_shapes(H, W))

    def call(want_map, want_value, want_layers):
        m = torch.full((n, H, W), -1.0, device=DEV) if want_map else None
        v = torch.full((n,), -1.0, device=DEV) if want_value else None
        d = torch.full((n, total), -1.0, device=DEV) if want_layers else None
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(lib.rnerf_lpips(a.data_ptr(), b.data_ptr(), n, H, W, w.data_ptr(), ptr(m), ptr(v), ptr(d), ws.data_ptr(), stream), "rnerf_lpips")
        torch.cuda.synchronize()
        return m, v, d
    m, _, _ = call(True, False, False)
    assert m.cpu().numpy().tobytes() == smap.tobytes()
    _, v, _ = call(False, True, False)
    assert v.cpu().numpy().tobytes() == value.tobytes()
    _, _, d = call(False, False, True)
    assert d.cpu().numpy().tobytes() == np.concatenate([x.reshape(n, -1) for x in layers], axis=1).tobytes()


def test_compute_lpips_takes_arrays_and_batches():
    from samplenerfro_amd import utils
    c = R.case("batch2")
    w = device_weights()
    smap, value, _ = run("batch2")
    got = utils.compute_lpips(c["img0"], c["img1"], w)                       # numpy in, device tensor out
    assert got.is_cuda and got.shape == (2,) and got.cpu().numpy().tobytes() == value.tobytes()
    one = utils.compute_lpips(T(c["img0"][1]), c["img1"][1], w)
    assert one.shape == () and float(one) == float(value[1])                 # a pair scores the same alone and in a batch
    m = utils.compute_lpips(c["img0"][0], T(c["img1"][0]), w, return_map=True)
    assert m.shape == (40, 52) and m.cpu().numpy().tobytes() == smap[0].tobytes()
    with pytest.raises(ValueError, match="31"):
        utils.compute_lpips(c["img0"][0][:30], c["img1"][0][:30], w)
    with pytest.raises(ValueError):
        utils.compute_lpips(c["img0"][0], c["img1"][0][:, :40], w)
