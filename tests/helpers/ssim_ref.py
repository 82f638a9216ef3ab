"""A numpy restatement of compute_ssim (rnerf/utils.py:404-471), the yardstick of rnerf_ssim.

`dtype=np.float64` is the exact-arithmetic reference (tests/golden/ssim_reference.npz pins it to the reference's own text);
`dtype=np.float32` evaluates the same formula in float32 as the reference does with x64 off, which sets the tolerance of the device
kernel (tests/test_gpu_ssim.py): blur(x^2) - mu^2 cancels, so float32 is itself far from float64 on smooth images."""
import numpy as np


def gaussian_filter(filter_size, filter_sigma):
    """rnerf/utils.py:435-439 in float64."""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    return filt / np.sum(filt)


def blur(z, filt):
    """Separable "valid" blur of [..., H, W, C]: along W, then along H (the window is symmetric: correlation = convolution)."""
    fs = len(filt)
    W = z.shape[-2] - fs + 1
    zw = sum(filt[k] * z[..., k:k + W, :] for k in range(fs))
    H = z.shape[-3] - fs + 1
    return sum(filt[k] * zw[..., k:k + H, :, :] for k in range(fs))


def ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False, dtype=np.float64):
    x, y = np.asarray(img0, dtype), np.asarray(img1, dtype)
    filt = gaussian_filter(filter_size, filter_sigma).astype(dtype)
    mu0, mu1 = blur(x, filt), blur(y, filt)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    sigma00 = blur(x ** 2, filt) - mu00
    sigma11 = blur(y ** 2, filt) - mu11
    sigma01 = blur(x * y, filt) - mu01
    sigma00 = np.maximum(dtype(0), sigma00)
    sigma11 = np.maximum(dtype(0), sigma11)
    sigma01 = np.sign(sigma01) * np.minimum(np.sqrt(sigma00 * sigma11), np.abs(sigma01))
    c1 = dtype((k1 * max_val) ** 2)
    c2 = dtype((k2 * max_val) ** 2)
    numer = (2 * mu01 + c1) * (2 * sigma01 + c2)
    denom = (mu00 + mu11 + c1) * (sigma00 + sigma11 + c2)
    ssim_map = numer / denom
    return ssim_map if return_map else np.mean(ssim_map, axis=(-3, -2, -1))
