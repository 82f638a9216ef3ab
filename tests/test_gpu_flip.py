"""rnerf_flip / ops.flip / utils.compute_flip on the device against the vectors the reference's own text computed
(tests/golden/flip_reference.npz) and, for sizes the fixture cannot hold, against the float64 restatement tests/helpers/flip_ref.py.

Tolerances are those of tests/test_flip_host.py.  Fixture cases: the floors stored in the file.  Larger pairs (all class A: the images
differ everywhere): the float32 rule of tests/test_gpu_ssim.py with flip_ref in float32 as the floor,
max|gpu - f64| <= 4 max|f32 - f64| + 1e-6 on the map and |mean_gpu - mean_f64| <= 2 mean|f32 - f64| + 1e-6.

Measured on an MI355X (ratio = map error / floor; bar 4 + 1e-6 / floor): see DESIGN.md 3.8."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_flip_reference as M      # noqa: E402
import flip_ref                      # noqa: E402
from flip_checks import check_against_fixture, identical_footprint, load_case      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HI, LO = M.PPD["hi"], M.PPD["lo"]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def gpu_flip(a, b, ppd, **kw):
    from samplenerfro_amd import utils
    return utils.compute_flip(T(a), T(b), ppd, **kw).cpu().numpy().astype(np.float64)


def smooth(shape, rng):
    H, W = shape[-3:-1]
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    ph = rng.uniform(0, 3, shape[:-3] + (1, 1))
    return np.stack([0.5 + 0.35 * np.sin(3 * xx + c + ph) * np.cos(2 * yy - c) for c in range(3)], -1).astype(np.float32)


def check_f32_rule(a, b, ppd, what):
    """The float32-restatement rule on map and mean; returns map error / floor (for the record)."""
    m64 = flip_ref.flip(a, b, ppd)
    m32 = flip_ref.flip(a, b, ppd, dtype=np.float32).astype(np.float64)
    mg = gpu_flip(a, b, ppd, return_map=True)
    assert mg.shape == m64.shape and not np.isnan(mg).any()
    e_gpu, e_32 = float(np.max(np.abs(mg - m64))), float(np.max(np.abs(m32 - m64)))
    meang = gpu_flip(a, b, ppd)
    mean64 = np.mean(m64, (-2, -1))
    assert meang.shape == mean64.shape
    d_mean = float(np.max(np.abs(meang - mean64)))
    mean_bound = 2 * float(np.mean(np.abs(m32 - m64))) + 1e-6
    print(f"{what}: map error {e_gpu:.3g} (float32 {e_32:.3g}, ratio {e_gpu / max(e_32, 1e-30):.3g}); mean error {d_mean:.3g} "
          f"(bound {mean_bound:.3g}); mean FLIP {float(np.mean(mean64)):.4f}")
    assert e_gpu <= 4 * e_32 + 1e-6, f"{what}: map error {e_gpu:.3g} vs float32's {e_32:.3g}"
    assert d_mean <= mean_bound, f"{what}: mean error {d_mean:.3g} > {mean_bound:.3g}"
    return e_gpu / max(e_32, 1e-30)


@pytest.mark.parametrize("key", M.keys())
def test_kernel_agrees_with_the_references_vectors(key):
    a, b, ppd, *_ = load_case(key)
    check_against_fixture(key, gpu_flip(a, b, ppd, return_map=True), gpu_flip(a, b, ppd))


@pytest.mark.parametrize("ppd", [LO, HI], ids=["lo", "hi"])
@pytest.mark.parametrize("shape", [(2, 37, 53, 3), (400, 400, 3), (800, 800, 3)], ids=["2x37x53", "400x400", "800x800"])
def test_larger_pairs_under_the_float32_rule(shape, ppd):
    rng = np.random.default_rng(sum(shape))
    if len(shape) == 4:                                  # one noise pair and one smooth pair, batched
        s = smooth(shape[1:], rng)
        a = np.stack([rng.uniform(0, 1, shape[1:]).astype(np.float32), s])
        b = np.stack([rng.uniform(0, 1, shape[1:]).astype(np.float32), s + 0.05 * rng.standard_normal(shape[1:])]).astype(np.float32)
    elif shape[0] == 400:
        a = smooth(shape, rng)
        b = (a + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    else:
        a, b = rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(0, 1, shape).astype(np.float32)
    check_f32_rule(a, np.clip(b, 0, 1), ppd, f"{shape} at {ppd:.4g} ppd")


@pytest.mark.parametrize("ppd", [LO, HI], ids=["lo", "hi"])
def test_example_photograph_against_a_noised_copy(ppd):
    img = np.load(os.path.join(ROOT, "tests", "golden", "example_image.npz"))["rgba_sum4"]
    a = (img[..., :3].astype(np.float32) / np.float32(1020.0))
    rng = np.random.default_rng(11)
    b = np.clip(a + 0.03 * rng.standard_normal(a.shape), 0, 1).astype(np.float32)
    if not np.all(np.any(a != b, axis=-1)):              # class A: every pixel differs (clipping may have undone the noise)
        b = np.where(np.any(a != b, axis=-1, keepdims=True), b, np.abs(a - np.float32(0.02))).astype(np.float32)
    assert np.all(np.any(a != b, axis=-1))
    check_f32_rule(a, b, ppd, f"photograph at {ppd:.4g} ppd")


@pytest.mark.parametrize("ppd", [LO, HI], ids=["lo", "hi"])
def test_an_image_against_itself_is_exactly_zero(ppd):
    from samplenerfro_amd import utils
    rng = np.random.default_rng(6)
    a = T(np.concatenate([rng.uniform(0, 1, (2, 70, 131, 3)), smooth((1, 70, 131, 3), rng)]))
    m = utils.compute_flip(a, a.clone(), ppd, return_map=True)
    assert m.shape == (3, 70, 131) and bool((m == 0).all())
    assert bool((utils.compute_flip(a, a.clone(), ppd) == 0).all())


@pytest.mark.parametrize("ppd", [LO, HI], ids=["lo", "hi"])
def test_a_half_identical_pair_is_exactly_zero_beyond_the_footprint(ppd):
    rng = np.random.default_rng(7)
    a = smooth((400, 400, 3), rng)
    b = a.copy()
    b[150:, 200:] = np.clip(b[150:, 200:] + 0.05 * rng.standard_normal((250, 200, 3)), 0, 1)
    m = gpu_flip(a, b, ppd, return_map=True)
    zero = identical_footprint(a, b, max(flip_ref.radii(ppd)))
    r = flip_ref.radii(ppd)[0]
    assert zero[:150 - r].all() and zero[:, :200 - r].all() and not zero[150:, 200:].any()
    assert np.all(m[zero] == 0.0)
    assert np.all(m[150:, 200:] > 0)


def test_nan_marks_the_spatial_footprint_of_one_image():
    rng = np.random.default_rng(5)
    a, b = rng.uniform(0, 1, (2, 40, 50, 3)).astype(np.float32), rng.uniform(0, 1, (2, 40, 50, 3)).astype(np.float32)
    b[1, 3, 30, 2] = np.nan
    for ppd, r in ((LO, 1), (HI, 10)):
        m = gpu_flip(a, b, ppd, return_map=True)
        want = np.zeros(m.shape, bool)
        want[1, max(0, 3 - r):3 + r + 1, 30 - r:30 + r + 1] = True
        assert np.array_equal(np.isnan(m), want)
        mean = gpu_flip(a, b, ppd)
        assert not np.isnan(mean[0]) and np.isnan(mean[1])


def test_two_calls_give_identical_bits():
    from samplenerfro_amd import utils
    rng = np.random.default_rng(8)
    a, b = T(rng.uniform(0, 1, (2, 300, 310, 3))), T(rng.uniform(0, 1, (2, 300, 310, 3)))
    for ppd in (LO, HI):
        m1, m2 = utils.compute_flip(a, b, ppd, return_map=True), utils.compute_flip(a, b, ppd, return_map=True)
        s1, s2 = utils.compute_flip(a, b, ppd), utils.compute_flip(a, b, ppd)
        assert torch.equal(m1, m2) and torch.equal(s1, s2)
        # the mean is the map's fp64 sum rounded to float32 once: within one float32 ulp of any other fp64 summation order
        assert float((s1 - m1.double().mean((-2, -1)).float()).abs().max()) <= 6e-8


def test_an_input_offset_by_four_bytes_gives_the_same_bits():
    from samplenerfro_amd import utils
    rng = np.random.default_rng(13)
    shape = (2, 37, 53, 3)
    a, b = T(rng.uniform(0, 1, shape)), T(rng.uniform(0, 1, shape))
    n = a.numel()
    buf_a, buf_b = torch.empty(n + 1, device=DEV), torch.empty(n + 3, device=DEV)
    ua, ub = buf_a[1:].view(shape), buf_b[3:].view(shape)
    ua.copy_(a); ub.copy_(b)
    assert ua.data_ptr() % 16 and ub.data_ptr() % 16
    for ppd in (LO, HI):
        assert torch.equal(utils.compute_flip(ua, ub, ppd, return_map=True), utils.compute_flip(a, b, ppd, return_map=True))
        assert torch.equal(utils.compute_flip(ua, ub, ppd), utils.compute_flip(a, b, ppd))


def test_compute_flip_shapes_and_inputs():
    from samplenerfro_amd import utils
    rng = np.random.default_rng(9)
    a = rng.uniform(0, 1, (2, 3, 20, 22, 3)).astype(np.float32)
    b = rng.uniform(0, 1, (2, 3, 20, 22, 3)).astype(np.float32)
    m64, m32 = flip_ref.flip(a, b, HI), flip_ref.flip(a, b, HI, dtype=np.float32)
    want, bound = np.mean(m64, (-2, -1)), 2 * float(np.mean(np.abs(m32 - m64))) + 1e-6           # the float32 rule on a mean
    s = utils.compute_flip(a[0, 0], b[0, 0])                                   # numpy in, the default pixels_per_degree
    assert isinstance(s, torch.Tensor) and s.is_cuda and s.shape == () and s.dtype == torch.float32
    assert abs(float(s) - want[0, 0]) <= bound
    assert utils.compute_flip(a[0], b[0]).shape == (3,)
    assert utils.compute_flip(T(a[:, 0]), b[:, 0]).shape == (2,)               # torch + numpy: numpy is uploaded beside the tensor
    assert utils.compute_flip(a[:, 0], torch.from_numpy(b[:, 0])).shape == (2,)   # numpy + CPU tensor
    r = utils.compute_flip(T(a), T(b))
    assert r.shape == (2, 3) and np.max(np.abs(r.cpu().numpy() - want)) <= bound
    assert utils.compute_flip(a, b, return_map=True).shape == (2, 3, 20, 22)
    assert utils.compute_flip(a.astype(np.float64), b.astype(np.float64), utils.FLIP_PPD_SUMMARY).dtype == torch.float32
    assert utils.compute_flip(a[0, 0, :1, :1], b[0, 0, :1, :1], return_map=True).shape == (1, 1)      # one pixel: all border
    with pytest.raises(ValueError):
        utils.compute_flip(T(a), T(b[:, :2]))
    with pytest.raises(ValueError):
        utils.compute_flip(T(a[..., :2]), T(b[..., :2]))
    from samplenerfro_amd import _lib
    with pytest.raises(_lib.RnerfError):
        utils.compute_flip(T(a), T(b), 200.0)                                  # radius 28: beyond the tile plan


def test_compute_flip_does_not_synchronise():
    from samplenerfro_amd import utils
    rng = np.random.default_rng(10)
    a, b = T(rng.uniform(0, 1, (400, 400, 3))), T(rng.uniform(0, 1, (400, 400, 3)))
    first = utils.compute_flip(a, b)
    torch.cuda.synchronize()
    torch.cuda._sleep(50_000_000)                      # keep the stream busy for tens of milliseconds
    s = utils.compute_flip(a, b)
    done = torch.cuda.Event()
    done.record()
    assert not done.query(), "compute_flip returned after the stream drained: it synchronised"
    torch.cuda.synchronize()
    assert torch.equal(s, first)


def test_time_per_800x800_frame():
    """Prints the time of one call; a new kernel has no earlier number to be held to, so no bar is asserted."""
    from samplenerfro_amd import ops
    rng = np.random.default_rng(12)
    a, b = T(rng.uniform(0, 1, (800, 800, 3))), T(rng.uniform(0, 1, (800, 800, 3)))
    for ppd in (LO, HI):
        for _ in range(10):
            ops.flip(a, b, pixels_per_degree=ppd)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(100):
            ops.flip(a, b, pixels_per_degree=ppd)
        t1.record()
        torch.cuda.synchronize()
        print(f"FLIP 800x800 at {ppd:.4g} ppd: {1e3 * t0.elapsed_time(t1) / 100:.1f} us per call (device events, 100 calls)")
