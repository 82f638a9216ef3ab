"""The compositing forward against the oracle at the widths the product launcher picks by itself: test_gpu_parity.test_composite holds
B = 200 (64 lanes per ray); here B = 1025 (16 lanes) and B = 8193 (4 lanes, 8193 = 16 * 512 + 1: a one-ray tail block).  The same inputs,
special rows and tolerances as test_composite (derived there: expf / log1pf against numpy, a few ulp per sample, sums of <= 33 terms)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ref_np as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no ROCm device is visible")
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _rows(pos, dirs, dist):
    """[B,S,.] oracle arrays -> sample-major float4 records."""
    B, S = dist.shape
    pd = np.concatenate([pos, dist[..., None]], -1).transpose(1, 0, 2)
    dr = np.concatenate([dirs, np.zeros((B, S, 1), F32)], -1).transpose(1, 0, 2)
    return np.ascontiguousarray(pd, F32), np.ascontiguousarray(dr, F32)


@pytest.mark.parametrize("B", [1025, 8193])
def test_composite_at_16_and_4_lanes_per_ray(B):
    from samplenerfro_amd import ops
    rng = np.random.default_rng(1)
    S = 33
    t = np.sort(rng.uniform(2, 6, (B, S)).astype(F32), -1)
    dirs = R.safe_l2_normalize(rng.standard_normal((B, S, 3)).astype(F32))
    pos = rng.standard_normal((B, S, 3)).astype(F32)
    raw = (3 * rng.standard_normal((B, S, 4))).astype(F32)
    raw[:5, :, 3] = -80.0      # sigma = 0 exactly -> acc = 0 -> dist = t_0 (nan_to_num quirk)
    raw[5:10, :, 3] = 60.0     # opaque
    raw[B - 1, :, 3] = -80.0   # the ray of the tail block too
    bk = rng.uniform(0, 1, (B, 3)).astype(F32)
    rgb = R.rgb_activation(raw[..., :3]); sig = R.sigma_activation(raw[..., 3:])
    pd, dr = _rows(pos, dirs, t)
    for white in (False, True):
        ref = R.volumetric_rendering(rgb, sig, t, dirs, white, bk)
        out = ops.composite(T(raw.transpose(1, 0, 2)), T(pd), T(dr), None, S, B, T(bk), white, want_weights=True, want_alpha=True)
        o = [x.cpu().numpy() for x in out]
        np.testing.assert_allclose(o[0], ref[0], atol=2e-6, rtol=0)              # rgb
        np.testing.assert_allclose(o[1], ref[1], atol=1e-5, rtol=2e-6)           # distance (a ratio)
        np.testing.assert_allclose(o[2], ref[2], atol=2e-6, rtol=0)              # acc
        np.testing.assert_allclose(o[5].T, ref[3], atol=1e-6, rtol=0)            # weights
        np.testing.assert_allclose(o[6].T, ref[4], atol=1e-6, rtol=0)            # alpha
        np.testing.assert_allclose(o[3], ref[5], atol=1e-6, rtol=0)              # trans
        np.testing.assert_allclose(o[4], ref[6], atol=1e-6, rtol=0)              # trans * bkgd
        assert np.all(o[1][:5] == t[:5, 0]) and o[1][B - 1] == t[B - 1, 0]
