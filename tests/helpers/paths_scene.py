"""What the bent-path GPU tests share: a 40 x 48 crop of the example scene's view (tests/golden fixtures; the set-up of
tests/test_gpu_evaluate_vis.py) around the object's silhouette, and a 12^3 ball grid with 70 rays for the device's own march."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

F32 = np.float32
S, F, P = 64, 128, 12
CROP = (slice(20, 60), slice(130, 178))            # 40 rows x 48 columns of the 400 x 400 view, across the object's upper edge
BALL_G, BALL_EXT, BALL_N, BALL_B = 12, 1.5, 24, 70


def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def example_crop():
    """-> dict(model, variables, rays: Rays of [40, 48, 3] device tensors, pixels: [40, 48, 3] device tensor)."""
    import torch
    import cases
    from samplenerfro_amd import evaluate, models, synthetic as syn, utils as U
    img = np.load(os.path.join(ROOT, "tests", "golden", "example_image.npz"))["rgba_sum4"]
    pixels = (img[..., :3].astype(F32) / F32(1020.0))
    _, _, counts = cases.load_example_obj()
    grid = cases.example_grid(counts).astype(F32)
    H = W = 400
    focal = 0.5 * W / math.tan(0.5 * cases.EXAMPLE_CAMERA_ANGLE_X)
    flags = U.default_flags(num_coarse_samples=S, num_fine_samples=F, num_path_samples=P, white_bkgd=False, use_online_sparsity=False,
                            randomized=True, near=2.0, far=6.0, batch_size=1024, bg_weight=0.025, bg_smooth_weight=1.0, bg_patch_size=128,
                            config="configs/example")
    seed = 3
    model, variables = models.construct_nerf(np.array([0, seed], np.uint32), None, flags, [128] * 3, [-1.5] * 3, [1.5] * 3, T(grid))
    pf = syn.init_params_flat(seed, fine=True)
    for k in ("coarse_mlp", "fine_mlp", "bkgd_mlp"):
        variables["flat"][k].copy_(T(pf[k]))
    view = next(iter(evaluate.device_views(pixels[None], np.asarray(cases.EXAMPLE_C2W, F32)[None], focal=focal, device=torch.device("cuda:0"))))
    rays = U.Rays(view["rays"].origins[CROP].contiguous(), None, view["rays"].viewdirs[CROP].contiguous(), None)
    return dict(model=model, variables=variables, rays=rays, pixels=view["pixels"][CROP].contiguous())


def ball():
    """-> dict(grid float32 [12, 12, 12], ndim, nmin, nmax, o, d: float32 [70, 3]): a smoothed ball of n = 1.5 and rays towards it."""
    from oracle import ref_np as O
    from samplenerfro_amd import synthetic as syn
    ndim, nmin, nmax = [BALL_G] * 3, [-BALL_EXT] * 3, [BALL_EXT] * 3
    grid = O.conv3d_normal(syn.scale_ior(syn.sphere_grid(BALL_G, BALL_EXT, 0.7), 0.5).reshape(-1, 1), ndim, 3, 1.0).reshape(ndim).astype(F32)
    o, d = syn.sphere_rays(BALL_B, seed=5, target_radius=1.3)
    k = 12                                              # the last 12 rays pass the ball at a distance, along x near the grid's long edges
    rng = np.random.default_rng(9)
    o[-k:] = np.stack([-4.0 * np.ones(k), rng.choice([-1.0, 1.0], k) * rng.uniform(1.3, 1.45, k),
                       rng.choice([-1.0, 1.0], k) * rng.uniform(1.3, 1.45, k)], -1)
    d[-k:] = (1.0, 0.0, 0.0)
    return dict(grid=grid, ndim=ndim, nmin=nmin, nmax=nmax, o=o.astype(F32), d=d.astype(F32))
