"""samplenerfro_amd.compare on the device against tests/helpers/compare_ref.py: rnerf_compare_sheet and rnerf_compare_strip byte for byte
and count for count on synthetic inputs, then compare_views end to end at the shapes of tests/golden/errmap_reference.npz.

Synthetic maps.  Every pair is seeded with the differences at which the classification can go wrong: 0, float32(1e-3) and its two
float32 neighbours (both orders), -0.0 against 0.0, +-inf against a finite value (both orders), equal infinities, NaN on either side.
Shapes: 1 x 1 in 1 x 1 (one thread, a 3-byte tail after nothing: every seeded pair in turn); 7 x 5, 9 x 6 and 3 x 6 in 9 x 6 (rows of
99 bytes: a thread's four bytes straddle rows, the tail is 3 bytes); K = 4 in 33 x 31; K = 4 in 800 x 800 (7547 steps of 1024 bytes
over the 2048 workgroups of the grid-stride loop) and one 701 x 1000 map (just over one pass of the loop, with a 3-byte tail in the second).

End to end.  Run A is the fixture's in_*_test, run B is A + 0.05 default_rng(7).standard_normal rounded to float32, both as 8-bit
images (A as the uint8 array a PNG reader returns, B as a float render, which compare_views quantises itself).
  - Against the helper fed with the device's own maps read back: bytes and counts exact.
  - Against the helper's classification of errmap_ref's float64 maps: a pixel may differ only if ||a - b| - 1e-3| <= 2 bound on the
    float64 maps, bound = max(4 e_ref, 1e-6), the map tolerance of tests/test_gpu_errmap.py (each map is within `bound` of float64, so
    |a - b| is within 2 bound; where |a - b| < 2 bound the order of a and b may flip too, but that is a tie on both sides).  The band
    must hold at most 1 % of a map, asserted on the float64 maps themselves, so that a change of inputs cannot hide a failure.  On
    the CPU the float64 maps put 1 of 957 and 1 of 3150 squared-error pixels and 0 of 437 and 1 of 2100 SSIM pixels in the band.
The tests print the band shares and the number of differing pixels."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import compare_ref as R               # noqa: E402
import errmap_ref as E                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CASES = ("29x33", "45x70")
T3 = F32(1e-3)
BELOW, ABOVE = np.nextafter(T3, F32(0)), np.nextafter(T3, F32(1))
NAN, INF = F32(np.nan), F32(np.inf)
# (a, b): the first 17 fit the smallest seeded map (3 x 6)
SEEDS = [(0.25, 0.25), (0.0, T3), (T3, 0.0), (0.0, BELOW), (0.0, ABOVE), (BELOW, 0.0), (ABOVE, 0.0), (-0.0, 0.0), (0.0, -0.0),
         (INF, 0.5), (-INF, 0.5), (0.5, INF), (0.5, -INF), (INF, INF), (-INF, -INF), (NAN, 0.5), (0.5, NAN), (INF, -INF), (NAN, NAN)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def seeded_pair(h, w, seed):
    """Two float32 maps [h, w]: uniform values whose differences straddle 1e-3, with SEEDS planted from the first element on."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, (h, w)).astype(F32)
    b = (a + rng.choice([F32(1e-4), F32(2e-3), F32(0.1)], (h, w)).astype(F32) * rng.standard_normal((h, w)).astype(F32)).astype(F32)
    fa, fb = a.reshape(-1), b.reshape(-1)
    for i, (x, y) in enumerate(SEEDS[:fa.size]):
        fa[i], fb[i] = x, y
    return a, b


def seeded_maps(shapes, seed):
    pairs = [seeded_pair(h, w, seed + k) for k, (h, w) in enumerate(shapes)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def check_win_loss(maps_a, maps_b, H, W):
    from samplenerfro_amd import compare
    frame, counts = compare.win_loss([T(m) for m in maps_a], maps_b, H, W)
    K = len(maps_a)
    assert frame.is_cuda and frame.dtype == torch.uint8 and tuple(frame.shape) == (H, K * (W + 5), 3)
    assert counts.is_cuda and counts.dtype == torch.int64 and tuple(counts.shape) == (K, 4)
    want = R.frame(maps_a, maps_b, H, W)
    got, got_counts = frame.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got_counts, R.counts(maps_a, maps_b)) and got_counts.sum(1).tolist() == [m.size for m in maps_a]
    for panel, a, b in zip(compare.panels(got, [m.shape for m in maps_a]), maps_a, maps_b):
        assert np.array_equal(panel, R.colorize(a, b))               # compare.py's per-metric PNGs are slices of the frame
    return got, got_counts


def test_one_pixel_every_seeded_pair():
    from samplenerfro_amd import compare
    colours = R.colours()
    for x, y in SEEDS:
        a, b = np.array([[x]], F32), np.array([[y]], F32)
        frame, counts = compare.win_loss([a], [T(b)], 1, 1)
        cls = int(R.classify(a, b)[0, 0])
        want = np.full((1, 6, 3), 255, np.uint8)
        want[0, 0] = colours[cls]
        assert np.array_equal(frame.cpu().numpy(), want) and np.array_equal(want, R.frame([a], [b], 1, 1)), (x, y)
        assert counts.cpu().numpy().tolist() == [[int(c == cls) for c in range(4)]], (x, y)


@pytest.mark.parametrize("H,W,shapes", [(9, 6, [(7, 5), (9, 6), (3, 6)]), (33, 31, [(33, 31), (23, 21), (33, 31), (1, 31)]),
                                        (800, 800, [(800, 800), (790, 790), (800, 800), (800, 800)]), (701, 1000, [(701, 1000)])])
def test_win_loss_bytes_and_counts_are_exact(H, W, shapes):
    maps_a, maps_b = seeded_maps(shapes, 11)
    _, counts = check_win_loss(maps_a, maps_b, H, W)
    assert (counts[:, [0, 1, 2]] > 0).all() and (counts[:, 3] >= 2).all()          # every class occurs in every map


def test_unaligned_out_no_counts_and_bit_stable_counts():
    from samplenerfro_amd import _lib, compare
    H, W, shapes = 9, 6, [(7, 5), (9, 6), (3, 6)]
    maps_a, maps_b = seeded_maps(shapes, 11)
    want, want_counts = R.frame(maps_a, maps_b, H, W), R.counts(maps_a, maps_b)
    assert want.shape[1] * 3 == 99 and want.size % 4 == 3           # rows of 99 bytes, a tail of 3
    frame, none = compare.win_loss(maps_a, maps_b, H, W, counts=False)
    assert none is None and np.array_equal(frame.cpu().numpy(), want)
    da, db = [T(m) for m in maps_a], [T(m) for m in maps_b]
    lib = _lib.load()
    buf = torch.zeros(want.size + 2, dtype=torch.uint8, device=DEV)
    unaligned = buf[1:-1].view(want.shape)                            # a frame that starts on an odd address
    counts = torch.full((3, 4), -7, dtype=torch.int64, device=DEV)    # the call clears it itself
    arr = lambda t, vals: (t * 3)(*vals)
    for _ in range(2):
        rc = lib.rnerf_compare_sheet(H, W, 3, arr(ctypes.c_void_p, [m.data_ptr() for m in da]), arr(ctypes.c_void_p, [m.data_ptr() for m in db]),
                                     arr(ctypes.c_int32, [h for h, _ in shapes]), arr(ctypes.c_int32, [w for _, w in shapes]), unaligned.data_ptr(),
                                     counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert np.array_equal(unaligned.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert int(buf[0]) == 0 and int(buf[-1]) == 0                     # nothing written before or after the frame
    with pytest.raises(_lib.RnerfError, match="no larger than the image"):
        compare.win_loss([torch.zeros((10, 6), device=DEV)], [torch.zeros((10, 6), device=DEV)], 9, 6)
    with pytest.raises(_lib.RnerfError, match="K must be"):
        compare.win_loss([torch.zeros((2, 2), device=DEV)] * 5, [torch.zeros((2, 2), device=DEV)] * 5, 9, 6)
    with pytest.raises(ValueError, match="one shape"):
        compare.win_loss([torch.zeros((2, 2), device=DEV)], [torch.zeros((2, 3), device=DEV)], 9, 6)


def strip_images(N, H, W, base):
    """N + 1 uint8 images [H, W, 3] of consecutive byte values (mod 256) from `base` on."""
    n = H * W * 3
    return [((np.arange(n) + base + i * n) % 256).astype(np.uint8).reshape(H, W, 3) for i in range(N + 1)]


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("H,W", [(5, 7), (33, 31)])
def test_strip_bytes_are_exact(N, H, W):
    from samplenerfro_amd import compare
    rects = [None, (2, 1, W - 4, H - 3), (0, 0, W - 2, H - 2), (2, 2, W - 2, H - 2), (0, 0, W, 1), (0, 0, 1, H), (0, 0, W, H)]
    seen = set()
    for base in range(0, 256, min(H * W * 3, 256)):                   # 5 x 7 x 3 = 105 bytes: three sets cover every byte value
        *images, ref = strip_images(N, H, W, base)
        seen |= set(images[0].reshape(-1).tolist())
        for rect in rects:
            got = compare.strip([T(im) for im in images], ref, rect)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (H, N * (W + 5) + W, 3)
            assert np.array_equal(got.cpu().numpy(), R.strip(images, ref, rect)), (base, rect)
        if base == 0:
            whole, none = compare.strip(images, ref, (0, 0, W, H)), compare.strip(images, ref)
            assert torch.equal(whole, none)                            # weight 1 is the identity on every byte
            assert np.array_equal(compare.strip(images, ref, (3, 0, 0, 2)).cpu().numpy(), none.cpu().numpy())      # w == 0: no rectangle
    assert seen == set(range(256))


def test_strip_floats_unaligned_out_and_errors():
    from samplenerfro_amd import _lib, compare
    H, W = 5, 7
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(F32)
    x[0, 0], x[0, 1, 0], x[1, 1] = [0.5, 254.999 / 255, 1.0], np.nan, [0.2, 1 / 255, 0.0]
    as_bytes = (np.clip(np.where(np.isnan(x), F32(0), x), 0., 1.) * 255.).astype(np.uint8)      # utils.save_img's conversion
    ref = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = compare.strip([x, T(as_bytes)], ref, (1, 1, 3, 2)).cpu().numpy()
    assert np.array_equal(got, R.strip([as_bytes, as_bytes], ref, (1, 1, 3, 2)))
    want = R.strip([as_bytes], ref, (1, 1, 3, 2))
    assert want.size % 4 == 1                                         # 57-byte rows: a tail of one byte
    lib = _lib.load()
    buf = torch.zeros(want.size + 2, dtype=torch.uint8, device=DEV)
    unaligned = buf[1:-1].view(want.shape)
    img, dref = T(as_bytes), T(ref)
    rc = lib.rnerf_compare_strip((ctypes.c_void_p * 1)(img.data_ptr()), 1, dref.data_ptr(), H, W, 1, 1, 3, 2, unaligned.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and np.array_equal(unaligned.cpu().numpy(), want) and int(buf[0]) == 0 and int(buf[-1]) == 0
    with pytest.raises(_lib.RnerfError, match="inside the image"):
        compare.strip([as_bytes], ref, (5, 0, 3, 2))
    with pytest.raises(_lib.RnerfError, match="N must be"):
        compare.strip([as_bytes] * 5, ref)
    with pytest.raises(ValueError, match="like the reference"):
        compare.strip([as_bytes[:4]], ref)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(ROOT, "tests", "golden", "errmap_reference.npz"))


@pytest.fixture(scope="module")
def runs(fix):
    """case -> (ground truth, run A as uint8, run B as a float render, both runs as the float32 images a PNG reader forms)."""
    out = {}
    for case in CASES:
        ref, a = fix[f"in_{case}_ref"], fix[f"in_{case}_test"]
        b = (a + 0.05 * np.random.default_rng(7).standard_normal(a.shape)).astype(F32)
        qa, qb = E.quantize8(a), E.quantize8(b)
        a8 = (qa * F32(255)).astype(np.uint8)
        assert np.array_equal(a8.astype(F32) / F32(255), qa)
        out[case] = (ref, a8, b, qa, qb)
    return out


@pytest.fixture(scope="module")
def compared(runs):
    """compare_views over both fixture shapes, once; and each run's device maps read back."""
    from samplenerfro_amd import compare
    views = [{"pixels": T(runs[c][0])} for c in CASES]
    res = compare.compare_views(views, [runs[c][1] for c in CASES], (T(runs[c][2]) for c in CASES), keep_frames=True, strips=True)
    maps = []
    for c in CASES:
        ref, _, _, qa, qb = runs[c]
        maps.append(tuple({k: v.cpu().numpy() for k, v in compare.metric_maps(ref, T(q)).items()} for q in (qa, qb)))
    return res, maps


def test_compare_views_equals_the_helper_on_the_devices_own_maps(runs, compared):
    from samplenerfro_amd import compare
    res, maps = compared
    names = compare.MAP_NAMES
    assert res["names"] == names and len(res["counts"]) == 2 and "mask_mode" not in res
    total = np.zeros((3, 4), np.int64)
    for i, case in enumerate(CASES):
        ref, a8, b, qa, qb = runs[case]
        H, W = ref.shape[:2]
        ma, mb = maps[i]
        assert res["shapes"][i] == [(H, W), (H - 10, W - 10), (H, W)]
        assert np.array_equal(ma["dssim"], F32(1) - np.clip(ma["ssim"], F32(0), F32(1))) and ma["dssim"].dtype == np.float32
        assert float(ma["dssim_value"]) == float(F32(1) - ma["ssim_value"])
        frame = res["frames"][i]
        assert frame.is_cuda and tuple(frame.shape) == (H, 3 * (W + 5), 3)
        assert np.array_equal(frame.cpu().numpy(), R.frame([ma[n] for n in names], [mb[n] for n in names], H, W))
        want_counts = R.counts([ma[n] for n in names], [mb[n] for n in names])
        assert res["counts"][i] == want_counts.tolist()
        total += want_counts
        for n in names:
            assert res["a"][n][i] == float(ma[n + "_value"]) and res["b"][n][i] == float(mb[n + "_value"]), n
        assert res["a"]["psnr"][i] > res["b"]["psnr"][i] and res["a"]["flip"][i] < res["b"]["flip"][i]      # B is A plus noise
        b8 = (qb * F32(255)).astype(np.uint8)
        ref8 = (np.clip(ref, 0., 1.) * 255.).astype(np.uint8)
        assert np.array_equal(res["strips"][i].cpu().numpy(), R.strip([a8, b8], ref8))
    for k, n in enumerate(names):
        assert res["shares"][n] == {c: float(total[k, j]) / float(total[k].sum()) for j, c in enumerate(compare.CLASSES)}
        assert res["shares"][n]["a"] > res["shares"][n]["b"] and res["shares"][n]["neither"] == 0.0
        assert res["mean_a"][n] == float(np.mean(np.array(res["a"][n]))) and res["mean_b"][n] == float(np.mean(np.array(res["b"][n])))


def classify64(a, b):
    """compare.py:221-223 on float64 maps."""
    d = np.abs(a - b)
    return np.where(d < 1e-3, R.CLASS_TIE, np.where(a <= b, R.CLASS_A, R.CLASS_B))


def test_compare_views_against_the_float64_maps(fix, runs, compared):
    from samplenerfro_amd import compare
    res, _ = compared
    colours = R.colours()
    for i, case in enumerate(CASES):
        ref, _, _, qa, qb = runs[case]
        got = compare.panels(res["frames"][i].cpu().numpy(), res["shapes"][i])
        for k, name, make in ((0, "psnr", lambda t: E.mse_map(ref, t)[0]), (1, "ssim", lambda t: 1.0 - np.clip(E.ssim_summary(ref, t)[0], 0.0, 1.0))):
            a64, b64 = make(qa), make(qb)
            bound = max(4 * float(fix[f"e_ref_{name}_{case}"]), 1e-6)
            band = np.abs(np.abs(a64 - b64) - 1e-3) <= 2 * bound
            differ = (got[k] != colours[classify64(a64, b64)]).any(-1)
            print(f"{case} {name}: {int(band.sum())} of {band.size} float64 pixels within {2 * bound:.3g} of the threshold "
                  f"({band.mean():.4f}); {int(differ.sum())} pixels differ from the float64 classification")
            assert band.mean() <= 0.01, (case, name)                   # a condition on the inputs
            assert not (differ & ~band).any(), (case, name, np.argwhere(differ & ~band)[:5])


def masks_for(case):
    """As tests/test_gpu_evaluate_masked.py: a 0 / 255 uint8 numpy disc for the first view, a 0 / 1 float device rectangle for the second."""
    if case == "29x33":
        yy, xx = np.mgrid[:29, :33]
        return (((yy - 14) ** 2 + (xx - 16) ** 2) < 8 ** 2).astype(np.uint8) * 255, (9, 7, 15, 15)
    rect = torch.zeros((45, 70), device=DEV)
    rect[5:40, 10:55] = 1.0
    return rect, (10, 5, 45, 35)


@pytest.mark.parametrize("mode,suffix", [("mask", "_mask"), ("crop", "_crop"), ("mask_crop", "_mask")])
def test_masked_and_cropped_views_and_their_files(runs, tmp_path, mode, suffix):
    from PIL import Image
    from samplenerfro_amd import compare
    views = [{"pixels": T(runs[c][0])} for c in CASES]
    masks = [masks_for(c)[0] for c in CASES]
    res = compare.compare_views(views, [runs[c][1] for c in CASES], [runs[c][2] for c in CASES], masks=masks, mask_mode=mode, out_dir=str(tmp_path),
                                name_b="noisy", save_output=True, strips=True, keep_frames=True)
    assert res["mask_mode"] == mode
    top = tmp_path / f"compare_noisy{suffix}"
    assert os.listdir(tmp_path) == [top.name]
    assert sorted(os.listdir(top)) == sorted([f"{n}_{i:03d}.png" for n in compare.MAP_NAMES for i in range(2)] + ["frame" + suffix, "strip" + suffix])
    for i, case in enumerate(CASES):
        ref, a8, _, qa, qb = runs[case]
        x, y, w, h = masks_for(case)[1]
        m = (torch.as_tensor(masks[i]).cpu().numpy() > 0)
        rows, cols = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
        assert (x, y, w, h) == (cols.min(), rows.min(), cols.max() + 1 - cols.min(), rows.max() + 1 - rows.min())
        H, W = (h, w) if mode != "mask" else ref.shape[:2]
        frame = res["frames"][i].cpu().numpy()
        assert frame.shape == (H, 3 * (W + 5), 3) and res["shapes"][i] == [(H, W), (H - 10, W - 10), (H, W)]
        assert np.asarray(res["counts"][i]).sum(1).tolist() == [H * W, (H - 10) * (W - 10), H * W]
        # compare.py:187-197 written out, then the unmasked path
        cut = lambda im: (im * m[..., None].astype(F32) if mode != "crop" else im)[(slice(y, y + h), slice(x, x + w)) if mode != "mask" else ...]
        ma, mb = (compare.metric_maps(np.ascontiguousarray(cut(ref)), np.ascontiguousarray(cut(q))) for q in (qa, qb))
        want, want_counts = compare.win_loss([ma[n] for n in compare.MAP_NAMES], [mb[n] for n in compare.MAP_NAMES], H, W)
        assert np.array_equal(frame, want.cpu().numpy()) and res["counts"][i] == want_counts.cpu().numpy().tolist()
        assert np.array_equal(np.asarray(Image.open(top / ("frame" + suffix) / f"frame_{i:03d}.png")), frame)
        for n, panel in zip(compare.MAP_NAMES, compare.panels(frame, res["shapes"][i])):
            assert np.array_equal(np.asarray(Image.open(top / f"{n}_{i:03d}.png")), panel), n
        strip = res["strips"][i].cpu().numpy()                         # the whole images; the rectangle in the crop modes
        b8 = (qb * F32(255)).astype(np.uint8)
        ref8 = (np.clip(ref, 0., 1.) * 255.).astype(np.uint8)
        assert np.array_equal(strip, R.strip([a8, b8], ref8, None if mode == "mask" else (x, y, w, h)))
        assert np.array_equal(np.asarray(Image.open(top / ("strip" + suffix) / f"strip_{i:03d}.png")), strip)
    if mode == "mask":
        assert np.asarray(res["counts"][0])[0, 1] >= 29 * 33 - int((masks[0] > 0).sum())     # outside the mask both errors are 0: ties


def test_lpips_gives_four_panels(runs, tmp_path):
    import lpips_ref
    from samplenerfro_amd import compare, lpips
    w = lpips_ref.weight_set(None)
    weights = lpips.from_tensors(w["convs"], w["biases"], w["lins"], device=DEV)
    ref, a8, b, qa, qb = runs["45x70"]
    res = compare.compare_views([{"pixels": ref}], [T(a8)], [b], lpips=weights, out_dir=str(tmp_path), save_output=True, keep_frames=True)
    assert res["names"] == compare.MAP_NAMES_LPIPS and res["shapes"][0] == [(45, 70), (35, 60), (45, 70), (45, 70)]
    frame = res["frames"][0].cpu().numpy()
    assert frame.shape == (45, 4 * 75, 3)
    ma, mb = ({k: v.cpu().numpy() for k, v in compare.metric_maps(ref, T(q), lpips=weights).items()} for q in (qa, qb))
    names = compare.MAP_NAMES_LPIPS
    assert np.array_equal(frame, R.frame([ma[n] for n in names], [mb[n] for n in names], 45, 70))
    assert res["counts"][0] == R.counts([ma[n] for n in names], [mb[n] for n in names]).tolist()
    assert res["a"]["lpips"] == [float(ma["lpips_value"])] and res["b"]["lpips"] == [float(mb["lpips_value"])]
    assert ma["lpips"].min() >= 0 and ma["lpips"].max() <= 1 and len({tuple(p) for p in compare.panels(frame, res["shapes"][0])[2].reshape(-1, 3)}) >= 2
    assert sorted(os.listdir(tmp_path / "compare_b")) == ["dssim_000.png", "flip_000.png", "frame", "lpips_000.png", "psnr_000.png"]


def test_compare_views_errors_name_the_view(runs):
    import lpips_ref
    from samplenerfro_amd import compare, lpips
    ref, a8, b, _, _ = runs["29x33"]
    views = [{"pixels": ref}] * 2
    with pytest.raises(ValueError, match="preds_b ran out at view 1"):
        compare.compare_views(views, [a8, a8], [b])
    with pytest.raises(ValueError, match="preds_a ran out at view 1"):
        compare.compare_views(views, iter([a8]), [b, b])
    with pytest.raises(ValueError, match="preds_a holds more than the 2 views"):
        compare.compare_views(views, [a8] * 3, [b] * 2)
    with pytest.raises(ValueError, match="masks ran out at view 1"):
        compare.compare_views(views, [a8] * 2, [b] * 2, masks=[np.ones((29, 33), np.uint8)], mask_mode="mask")
    with pytest.raises(ValueError, match="go together"):
        compare.compare_views(views, [a8] * 2, [b] * 2, mask_mode="crop")
    with pytest.raises(ValueError, match="view 0.*preds_b"):
        compare.compare_views(views, [a8] * 2, [b[:20]] * 2)
    with pytest.raises(ValueError, match="view 0.*SSIM window"):
        compare.compare_views([{"pixels": ref[:10]}], [a8[:10]], [b[:10]])
    tiny = np.zeros((29, 33), np.uint8)
    tiny[3:8, 2:30] = 1
    with pytest.raises(ValueError, match="view 0.*SSIM window"):
        compare.compare_views(views[:1], [a8], [b], masks=[tiny], mask_mode="crop")
    w = lpips_ref.weight_set(None)
    weights = lpips.from_tensors(w["convs"], w["biases"], w["lins"], device=DEV)
    with pytest.raises(ValueError, match="view 0.*LPIPS needs at least 31 x 31"):
        compare.compare_views(views[:1], [a8], [b], lpips=weights)
    with pytest.raises(ValueError, match="save_output needs out_dir"):
        compare.compare_views(views[:1], [a8], [b], save_output=True)
