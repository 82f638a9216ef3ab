"""A seeded writer of tiny scene directories in the three formats samplenerfro_amd.datasets opens (PIL and json only).

write_blender / write_opencv / write_nsvf(directory, ...) write 3 train and 2 test views of 8 x 12 pixels (RGBA; RGB for one OpenCV
variant) with camera-to-world matrices whose rotations are not trivial, and return the uint8 arrays they wrote per split, in file order.
The alpha channel holds 0, 255 and values in between.  tests/golden/make_scene_loader_reference.py runs the reference's loaders on exactly
these directories; the tests compare this project's loaders against that file and against the arrays returned here."""
import json
import os

import numpy as np
from PIL import Image

H, W = 8, 12
SPLITS = {"train": 3, "test": 2}
CAMERA_ANGLE_X = 0.6911112070083618
CAM_MAT = [[23.25, 0.0, 6.5], [0.0, 22.75, 3.75], [0.0, 0.0, 1.0]]
NSVF_INTRINSICS = (21.5, 6.0, 4.0, 0.0)


def _image(rng, channels, h=H, w=W):
    im = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    if channels == 4:
        a = im[..., 3]
        a[: h // 2, : w // 3] = 0            # a transparent block, an opaque block, random in between; whole 2 x 2 cells of both
        a[h // 2:, 2 * w // 3:] = 255
        a[0, w - 1], a[h - 1, 0] = 0, 255
    im[1, 1, :3], im[2, 2, :3] = 0, 255
    return im


def _pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = q.astype(np.float32)
    m[:3, 3] = rng.uniform(-3, 3, 3).astype(np.float32)
    return m


def _save(path, im):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(im).save(path, "PNG")      # [h, w, 4] uint8 -> RGBA, [h, w, 3] -> RGB


def _write_transforms(directory, seed, channels, name_of, extra, size=(H, W), frames=None):
    rng = np.random.default_rng(seed)
    out = {}
    for split, n in (frames or SPLITS).items():
        ims, fr = [], []
        for i in range(n):
            im, pose = _image(rng, channels, *size), _pose(rng)
            file_path, fname = name_of(split, i)
            _save(os.path.join(directory, fname), im)
            ims.append(im)
            fr.append({"file_path": file_path, "transform_matrix": [[float(v) for v in row] for row in pose]})
        with open(os.path.join(directory, f"transforms_{split}.json"), "w") as fp:
            json.dump(dict(extra, frames=fr), fp)
        out[split] = np.stack(ims)
    return out


def write_blender(directory, seed=11, channels=4, size=(H, W), frames=None):
    """transforms_{train,test}.json with camera_angle_x; file_path carries no extension (./train/r_0 -> train/r_0.png)."""
    return _write_transforms(directory, seed, channels, lambda s, i: (f"./{s}/r_{i}", os.path.join(s, f"r_{i}.png")),
                             {"camera_angle_x": CAMERA_ANGLE_X}, size, frames)


def write_opencv(directory, seed=12, channels=4):
    """transforms_{train,test}.json with cam_mat; file_path is the file's name as it is."""
    return _write_transforms(directory, seed, channels, lambda s, i: (f"imgs/{s}_{i:03d}.png",) * 2, {"cam_mat": CAM_MAT})


def write_nsvf(directory, seed=13, channels=4):
    """intrinsics.txt, rgb/{0,2}_NNNN.png and pose/{0,2}_NNNN.txt (prefix 0 = train, 2 = test)."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(directory, "pose"), exist_ok=True)
    with open(os.path.join(directory, "intrinsics.txt"), "w") as fp:
        fp.write(" ".join(repr(v) for v in NSVF_INTRINSICS) + "\n0.0 0.0 0.0\n")
    out = {}
    for split, n in SPLITS.items():
        ims = []
        for i in range(n):
            im, pose = _image(rng, channels), _pose(rng)
            stem = f"{dict(train=0, test=2)[split]}_{i:04d}"
            _save(os.path.join(directory, "rgb", stem + ".png"), im)
            np.savetxt(os.path.join(directory, "pose", stem + ".txt"), pose, fmt="%.9g")
            ims.append(im)
        out[split] = np.stack(ims)
    return out


def write_masks(directory, dataset, seed=14, size=(H, W)):
    """mask_<name>.png (0 / 255, mode L) beside every frame of a Blender or OpenCV scene written above -> {split: uint8 [n, H, W]}."""
    rng = np.random.default_rng(seed)
    out = {}
    for split in SPLITS:
        with open(os.path.join(directory, f"transforms_{split}.json")) as fp:
            frames = json.load(fp)["frames"]
        ms = []
        for f in frames:
            d, name = os.path.split(f["file_path"])
            m = (rng.integers(0, 2, size, dtype=np.uint8) * 255).astype(np.uint8)
            Image.fromarray(m).save(os.path.join(directory, d, "mask_" + (name if dataset == "blender" else name[:-4]) + ".png"), "PNG")
            ms.append(m)
        out[split] = np.stack(ms)
    return out


def prepare_reference(u8, factor=1, white_bkgd=False):
    """The definition of rnerf_images_prepare in numpy float32 (include/rnerf.h): uint8 [n, H, W, C] -> float32 [n, H / factor, W / factor, 3]."""
    f32 = np.float32
    u8 = np.asarray(u8)
    n, h, w, c = u8.shape
    if factor == 2:
        s = u8.astype(np.uint32).reshape(n, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4))
        x = s.astype(f32) / f32(1020.0)
    else:
        x = u8.astype(f32) / f32(255.0)
    if white_bkgd:
        return x[..., :3] * x[..., 3:4] + (f32(1.0) - x[..., 3:4])
    return np.ascontiguousarray(x[..., :3])
