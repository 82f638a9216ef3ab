"""Scenes and batches: the reference's rnerf/datasets.py without JAX and cv2, with the views resident on the device.

THE BATCH SAMPLER.  Reference: `Dataset.__init__ / run / __next__` (:59-119: a daemon thread that keeps a queue of 3
batches), `_train_init` (:123-145) and `_next_train` (:151-205).  The reference keeps the rays of every view as host arrays, draws ray
indices with numpy's global generator and indexes images and rays on the host; every batch is then shipped to the devices (`utils.shard`).

Here only the DRAW stays on the host — the same numpy calls in the same order, so a seeded run draws the reference's indices — in the same
kind of prefetch thread (a draw without replacement over 640 000 pixels is a 5 ms permutation, as in the reference).  The GATHER is one device
op (`rnerf_sample_batch`, csrc/render.hip): pixels from the resident image tensor, rays generated on the fly for exactly the drawn pixels
with the arithmetic of `rnerf_generate_rays` (bit-identical to indexing the reference's ray arrays, tests/test_gpu_batcher.py).  A training
loop then has no per-step host tensor work: 8 B per ray of indices go up, nothing comes down.

THE SCENE LOADERS.  Reference: `get_dataset` (:34-35), `Blender / NSVF / OpenCV._load_renderings` (:334-464), `Dataset._next_test`
(:202-213) and `OpenCV._next_test` (:466-484).  The host side follows them line by line: which JSON, which frames, which files, the camera.
The pixels do not become floats on the host: the PNGs are decoded (PIL, a small thread pool) to uint8, uploaded as uint8 in chunks of views
and turned into the float32 [n, h, w, 3] tensor by one kernel (`rnerf_images_prepare`, csrc/images.hip: / 255, the 2 x 2 area filter of
`factor: 2`, the composite over white).  No ray array is made at all: the train split hands the tensor to DeviceBatcher,
the val / test splits generate each view's rays when it is asked for (`ops.generate_rays`, what evaluate.device_views yields).
LLFF (NDC rays, spiral paths) and render_path are not built.
"""
from __future__ import annotations

import json
import os
import queue
import threading
from glob import glob
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .utils import Rays


class DeviceBatcher(threading.Thread):
    """`Dataset(split="train")` of the reference for views that are already decoded: next(batcher) -> {"pixels", "rays", "env_rays"}.

    images [n, H, W, C] float32 in [0, 1] (C = 3; the reference composites RGBA over white / black before, datasets.py:352-361),
    camtoworlds [n, 3, 4] (or [n, 4, 4]); focal= (Blender model, :216-242) or cam_mat= (OpenCV, :486-518).  rng: the numpy generator the
    draws come from — `np.random` (the module: the reference's global generator, seed it like train.py:188 does) or a RandomState.
    prefetch=0 draws in the calling thread (deterministic interleaving with other users of the generator: the tests)."""

    def __init__(self, images, camtoworlds, *, batch_size: int, device, focal: Optional[float] = None, cam_mat=None, pixel_center: bool = True,
                 batching: str = "single_image", patch_size: int = 0, precrop_iters: int = 0, precrop_frac: float = 0.5, rng=np.random,
                 prefetch: int = 3):
        super().__init__(daemon=True)
        if batching not in ("single_image", "all_images"):
            raise NotImplementedError(f"{batching} batching strategy is not implemented.")        # datasets.py:144-145
        if (focal is None) == (cam_mat is None):
            raise ValueError("give focal= (Blender camera) or cam_mat= (OpenCV camera)")
        img = torch.as_tensor(np.asarray(images, np.float32) if not isinstance(images, torch.Tensor) else images, dtype=torch.float32)
        if img.dim() != 4:
            raise ValueError("images must be [n, H, W, C]")
        self.n_examples, self.h, self.w, self.channels = (int(v) for v in img.shape)
        self.images = img.to(device).contiguous()
        c2w = np.asarray(camtoworlds, np.float32)[:, :3, :4]
        if c2w.shape != (self.n_examples, 3, 4):
            raise ValueError("camtoworlds must be [n, 3, 4] or [n, 4, 4]")
        self.camtoworlds = torch.from_numpy(np.ascontiguousarray(c2w)).to(device)
        self.camera = dict(focal=focal, cam_mat=cam_mat, pixel_center=pixel_center)
        self.batch_size, self.batching, self.patch_size = int(batch_size), batching, int(patch_size)
        self.precrop_iters, self.precrop_frac = int(precrop_iters), float(precrop_frac)
        self.train_it = 0
        self.rng = rng
        self.device = torch.device(device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.queue: "queue.Queue" = queue.Queue(max(int(prefetch), 1))
        self._threaded = prefetch > 0
        if self._threaded:
            self.start()

    # ---- the draw: numpy calls of _next_train, in its order --------------------------------------------------------------------------
    def _crop_coords(self):
        dH = int(self.h // 2 * self.precrop_frac)
        dW = int(self.w // 2 * self.precrop_frac)
        return np.arange(self.h * self.w).reshape(self.h, self.w)[(self.h // 2 - dH):(self.h // 2 + dH), (self.w // 2 - dW):(self.w // 2 + dW)]

    def draw(self) -> Dict[str, Any]:
        """One batch as INDICES: {"ray_indices": int64 [B] flat over (image, row, column), "env_indices": int64 [ps, ps] or None}."""
        hw = self.h * self.w
        if self.batching == "all_images":
            ray_indices = self.rng.choice(self.n_examples * hw, (self.batch_size,), replace=False)
        else:
            image_index = self.rng.randint(0, self.n_examples, ())
            if self.train_it < self.precrop_iters:
                ray_indices = self.rng.choice(self._crop_coords().reshape(-1), (self.batch_size,), replace=False)
            else:
                ray_indices = self.rng.choice(hw, (self.batch_size,), replace=False)
            ray_indices = ray_indices.astype(np.int64) + int(image_index) * hw
        env = None
        if self.patch_size > 0:
            image_index = self.rng.randint(0, self.n_examples, ())
            ps = self.patch_size
            if self.train_it < self.precrop_iters:
                coords = self._crop_coords()
                pH, pW = coords.shape
                x = self.rng.randint(low=0, high=pW - ps)
                y = self.rng.randint(low=0, high=pH - ps)
            else:
                coords = np.arange(hw).reshape(self.h, self.w)
                x = self.rng.randint(low=0, high=self.w - ps)
                y = self.rng.randint(low=0, high=self.h - ps)
            env = coords[y:(y + ps), x:(x + ps)].astype(np.int64) + int(image_index) * hw
        self.train_it += 1
        return {"ray_indices": np.ascontiguousarray(ray_indices, np.int64), "env_indices": env}

    # ---- the gather: one device op per ray set ------------------------------------------------------------------------------------------
    def gather(self, drawn: Dict[str, Any]) -> Dict[str, Any]:
        idx = torch.from_numpy(drawn["ray_indices"]).to(self.device, non_blocking=True)
        o, d, v, pix = ops.sample_batch(self.camtoworlds, self.images, idx, self.h, self.w, bad_count=self._bad, want_directions=True, **self.camera)
        env_rays = None
        if drawn["env_indices"] is not None:
            e = torch.from_numpy(np.ascontiguousarray(drawn["env_indices"].reshape(-1))).to(self.device, non_blocking=True)
            eo, ed, ev, _ = ops.sample_batch(self.camtoworlds, None, e, self.h, self.w, bad_count=self._bad, want_directions=True, **self.camera)
            shp = tuple(drawn["env_indices"].shape) + (3,)
            env_rays = Rays(eo.reshape(shp), ed.reshape(shp), ev.reshape(shp), None)
        return {"pixels": pix, "rays": Rays(o, d, v, None), "env_rays": env_rays}

    def run(self):
        while True:
            self.queue.put(self.draw())

    def __iter__(self):
        return self

    def __next__(self) -> Dict[str, Any]:
        return self.gather(self.queue.get() if self._threaded else self.draw())

    def out_of_range_indices(self) -> int:
        """Indices outside [0, n * H * W) met so far (reads a device counter: synchronises).  Always 0 for draws made here."""
        return int(self._bad.item())

    @property
    def size(self):
        return self.n_examples


# ---- scene loaders ----------------------------------------------------------------------------------------------------------------------
DECODE_WORKERS = 8                      # PNG decoding threads (PIL releases the GIL in zlib); a constant, not the machine's core count
UPLOAD_CHUNK_BYTES = 64 << 20           # decoded uint8 bytes per upload: a chunk of views is decoded while the one before is converted


class SceneIndex:
    """What `_load_renderings` knows before it opens an image: files [n] (absolute or data_dir-relative as joined there), camtoworlds
    float32 [n, 4, 4], the camera (camera_angle_x for Blender — its focal needs the image width —, focal for NSVF, cam_mat for OpenCV),
    factor 1 | 2 as rnerf_images_prepare takes it, white_bkgd, and for the mask files each frame's file_path."""

    def __init__(self, dataset, files, camtoworlds, *, factor=1, white_bkgd=False, camera_angle_x=None, focal=None, cam_mat=None, frame_paths=None):
        self.dataset, self.files, self.camtoworlds = dataset, list(files), camtoworlds
        self.factor, self.white_bkgd = int(factor), bool(white_bkgd)
        self.camera_angle_x, self.focal, self.cam_mat, self.frame_paths = camera_angle_x, focal, cam_mat, frame_paths

    def camera(self, w: int) -> Dict[str, Any]:
        """focal= or cam_mat= for an image of (loaded) width w."""
        if self.cam_mat is not None:
            return {"cam_mat": self.cam_mat}
        if self.camera_angle_x is not None:
            return {"focal": .5 * w / np.tan(.5 * self.camera_angle_x)}                     # datasets.py:368-369, with the halved w
        return {"focal": self.focal}


def _stack_cams(cams) -> np.ndarray:
    return np.stack(cams, axis=0) if cams else np.zeros((0, 4, 4), np.float32)


def _transforms(split: str, flags) -> dict:
    with open(os.path.join(flags.data_dir, "transforms_{}.json".format("train" if flags.eval_train else split)), "r") as fp:
        return json.load(fp)


def _check_split(split: str) -> None:
    if split not in ("train", "val", "test"):
        raise ValueError("the split argument should be either \"train\" or \"val\" or \"test\", set to {} here.".format(split))


def blender_index(split: str, flags) -> SceneIndex:
    """Blender._load_renderings (datasets.py:334-370) up to the pixels."""
    _check_split(split)
    if flags.render_path:
        raise ValueError("render_path cannot be used for the blender dataset.")
    if flags.factor != 2 and flags.factor > 0:
        raise ValueError("Blender dataset only supports factor=0 or 2, {} set.".format(flags.factor))
    meta = _transforms(split, flags)
    frames = [meta["frames"][i] for i in range(0, len(meta["frames"]), flags.skip_frames)]
    return SceneIndex("blender", [os.path.join(flags.data_dir, f["file_path"] + ".png") for f in frames],
                      _stack_cams([np.array(f["transform_matrix"], dtype=np.float32) for f in frames]), factor=2 if flags.factor == 2 else 1,
                      white_bkgd=flags.white_bkgd, camera_angle_x=float(meta["camera_angle_x"]), frame_paths=[f["file_path"] for f in frames])


def opencv_index(split: str, flags) -> SceneIndex:
    """OpenCV._load_renderings (datasets.py:429-464) up to the pixels: file_path as given, cam_mat from the JSON, no factor."""
    _check_split(split)
    if flags.render_path:
        raise ValueError("render_path cannot be used for the opencv dataset.")
    if flags.factor > 0:
        raise ValueError("Opencv dataset does not support factor, {} set.".format(flags.factor))
    meta = _transforms(split, flags)
    frames = [meta["frames"][i] for i in range(0, len(meta["frames"]), flags.skip_frames)]
    return SceneIndex("opencv", [os.path.join(flags.data_dir, f["file_path"]) for f in frames],
                      _stack_cams([np.array(f["transform_matrix"], dtype=np.float32) for f in frames]), white_bkgd=flags.white_bkgd,
                      cam_mat=meta["cam_mat"], frame_paths=[f["file_path"] for f in frames])


def nsvf_index(split: str, flags) -> SceneIndex:
    """NSVF._load_renderings (datasets.py:376-423) up to the pixels: intrinsics.txt, rgb/{0,1,2}_*.png, pose/*.txt with the Y and Z axes
    flipped; the focal halves with factor 2.  (skip_frames and eval_train are not read there.)"""
    _check_split(split)
    if flags.render_path:
        raise ValueError("render_path cannot be used for the nsvf dataset.")
    if flags.factor != 2 and flags.factor > 0:
        raise ValueError("NSVF dataset only supports factor=0 or 2, {} set.".format(flags.factor))
    prefix = {"train": 0, "val": 1, "test": 2}[split]
    with open(os.path.join(flags.data_dir, "intrinsics.txt"), "r") as fp:
        f, _cx, _cy, _ = map(float, fp.readline().split())
    imgfiles = sorted(glob(os.path.join(flags.data_dir, "rgb", f"{prefix}_*.png")))
    camfiles = sorted(glob(os.path.join(flags.data_dir, "pose", f"{prefix}_*.txt")))
    if len(camfiles) < len(imgfiles):
        raise ValueError(f"{flags.data_dir}: {len(imgfiles)} images but {len(camfiles)} poses for split {split!r}")
    cams = []
    for i in range(len(imgfiles)):
        cam = np.loadtxt(camfiles[i], dtype=np.float32)
        cam[:3, 1:3] *= -1                                                                  # flip Y, Z axes
        cams.append(cam)
    if flags.factor == 2:
        f *= 0.5
    return SceneIndex("nsvf", imgfiles, _stack_cams(cams), factor=2 if flags.factor == 2 else 1, white_bkgd=flags.white_bkgd, focal=f)


def _llff_index(split: str, flags) -> SceneIndex:
    raise NotImplementedError("the llff dataset is not built: no shipped config uses it, and its NDC rays (convert_to_ndc, the spiral and "
                              "spherical render paths) have no kernel here")


INDEXERS = {"blender": blender_index, "opencv": opencv_index, "nsvf": nsvf_index, "llff": _llff_index}


def _decode(fname: str) -> np.ndarray:
    """One PNG as the uint8 array PIL decodes it to ([H, W, 3] or [H, W, 4]; the reference converts the same array to float32)."""
    from PIL import Image
    with open(fname, "rb") as imgin:
        a = np.asarray(Image.open(imgin))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{fname}: need an 8-bit RGB or RGBA image, got {a.dtype} {a.shape}")
    return a


def decode_views(files: Sequence[str], pool=None, expect=None) -> np.ndarray:
    """uint8 [n, H, W, C] of `files`, decoded in `pool` (None: a pool of its own).  Every image must have one shape (`expect`, or the
    first file's): mixed sizes or channel counts within a scene are a ValueError, as np.stack makes them in the reference."""
    from concurrent.futures import ThreadPoolExecutor
    if pool is None:
        with ThreadPoolExecutor(max_workers=max(1, min(DECODE_WORKERS, len(files)))) as own:
            return decode_views(files, own, expect)
    return _stack_decoded(files, list(pool.map(_decode, files)), expect)


def _stack_decoded(files, arrays: List[np.ndarray], expect=None) -> np.ndarray:
    if not arrays:
        raise ValueError("no images to load")
    shape = tuple(expect) if expect is not None else arrays[0].shape
    for fname, a in zip(files, arrays):
        if a.shape != shape:
            raise ValueError(f"{fname}: image of shape {a.shape} in a scene of {shape} images: every view must have one size and channel count")
    return np.stack(arrays, axis=0)


def load_images(index: SceneIndex, device) -> torch.Tensor:
    """The views of `index` as the resident float32 [n, h, w, 3] tensor: decode -> upload uint8 -> rnerf_images_prepare, chunk by chunk,
    the next chunk decoding while this one is converted.  No float image exists on the host."""
    from concurrent.futures import ThreadPoolExecutor
    files = index.files
    if not files:
        raise ValueError("the scene has no frames for this split")
    device = torch.device(device)
    with ThreadPoolExecutor(max_workers=min(DECODE_WORKERS, len(files))) as pool:
        first = pool.submit(_decode, files[0])
        shape = first.result().shape
        H, W, C = shape
        if index.factor == 2 and (H % 2 or W % 2):
            raise ValueError(f"{files[0]}: factor 2 halves exactly; a {H} x {W} image has an odd side")
        if index.white_bkgd and C != 4:
            raise ValueError(f"{files[0]}: white_bkgd composites over the alpha channel; the image has {C} channels")
        per = max(1, UPLOAD_CHUNK_BYTES // (H * W * C))
        chunks = [(i, min(i + per, len(files))) for i in range(0, len(files), per)]
        submit = lambda c: [first if j == 0 else pool.submit(_decode, files[j]) for j in range(*c)]
        out = torch.empty((len(files), H // index.factor, W // index.factor, 3), dtype=torch.float32, device=device)
        pending = submit(chunks[0])
        for k, (i, j) in enumerate(chunks):
            futures, pending = pending, (submit(chunks[k + 1]) if k + 1 < len(chunks) else None)
            u8 = _stack_decoded(files[i:j], [f.result() for f in futures], shape)
            ops.images_prepare(torch.from_numpy(u8).to(device), index.factor, index.white_bkgd, out=out[i:j])
    return out


class SceneDataset:
    """`Dataset(split, args)` of the reference (datasets.py:61-127) over a loaded scene: an iterator of batches with `size` and `peek()`.

    split "train": wraps a DeviceBatcher built from the flags (`batcher`; next() is its next()).  "val" / "test": next() is `_next_test`
    (:202-213): {"pixels": [h, w, 3], "rays": Rays(origins, None, viewdirs, None)} of view `test_it`, wrapping round; the rays are made
    per view by ops.generate_rays, exactly what evaluate.device_views yields, so evaluate.evaluate takes the dataset as its views (bound it
    with itertools.islice(dataset, dataset.size): like the reference's, the iterator never ends)."""

    indexer = None

    def __init__(self, split: str, flags, device=None, rng=np.random, prefetch: int = 3):
        from . import distributed
        self.split = split
        self.index = type(self).indexer(split, flags)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.images = load_images(self.index, self.device)
        self.n_examples, self.h, self.w = (int(v) for v in self.images.shape[:3])
        self.resolution = self.h * self.w
        self.camtoworlds = self.index.camtoworlds
        self.camera = self.index.camera(self.w)
        self.focal, self.cam_mat = self.camera.get("focal"), self.camera.get("cam_mat")
        self.use_pixel_centers = bool(flags.use_pixel_centers)
        self.precrop_iters, self.precrop_frac = int(flags.precrop_iters), float(flags.precrop_frac)
        self.test_it = 0
        self._peeked = None
        self.batcher = None
        if split == "train":
            self.batcher = DeviceBatcher(self.images, self.camtoworlds, batch_size=int(flags.batch_size) // distributed.world()[1], device=self.device,
                                         pixel_center=self.use_pixel_centers, batching=flags.batching, patch_size=int(flags.bg_patch_size),
                                         precrop_iters=self.precrop_iters, precrop_frac=self.precrop_frac, rng=rng, prefetch=prefetch, **self.camera)

    def _test_window(self):
        """(row0, row1, col0, col1) of a test view: all of it (Dataset._next_test)."""
        return 0, self.h, 0, self.w

    def _next_test(self) -> Dict[str, Any]:
        idx = self.test_it
        self.test_it = (self.test_it + 1) % self.n_examples
        r0, r1, c0, c1 = self._test_window()
        o, _, v = ops.generate_rays(self.camtoworlds[idx], self.h, self.w, self.device, pixel_center=self.use_pixel_centers, rows=(r0, r1), **self.camera)
        pix = self.images[idx, r0:r1]
        if (c0, c1) != (0, self.w):
            o, v, pix = o[:, c0:c1].contiguous(), v[:, c0:c1].contiguous(), pix[:, c0:c1].contiguous()
        return {"pixels": pix, "rays": Rays(o, None, v, None)}

    def _produce(self) -> Dict[str, Any]:
        return next(self.batcher) if self.batcher is not None else self._next_test()

    def __iter__(self):
        return self

    def __next__(self) -> Dict[str, Any]:
        if self._peeked is not None:
            x, self._peeked = self._peeked, None
            return x
        return self._produce()

    def peek(self) -> Dict[str, Any]:
        """The batch the next next() returns, without consuming it (datasets.py:105-115)."""
        if self._peeked is None:
            self._peeked = self._produce()
        return self._peeked

    @property
    def size(self):
        return self.n_examples


class Blender(SceneDataset):
    """Blender Dataset (datasets.py:331-370)."""
    indexer = staticmethod(blender_index)


class NSVF(SceneDataset):
    """NSVF Dataset (datasets.py:373-423)."""
    indexer = staticmethod(nsvf_index)


class OpenCV(SceneDataset):
    """OpenCV Dataset (datasets.py:426-518)."""
    indexer = staticmethod(opencv_index)

    def _test_window(self):
        """OpenCV._next_test (datasets.py:466-484): the central crop of the test views, precrop_frac of each half side while precrop_iters
        is set (dolphin.yaml), pixels and rays alike."""
        if self.precrop_iters > 0:
            dH = int(self.h // 2 * self.precrop_frac)
            dW = int(self.w // 2 * self.precrop_frac)
        else:
            dH = self.h // 2
            dW = self.w // 2
        return self.h // 2 - dH, self.h // 2 + dH, self.w // 2 - dW, self.w // 2 + dW


class _LLFF:
    def __init__(self, split, flags, *a, **k):
        _llff_index(split, flags)


dataset_dict = {"blender": Blender, "llff": _LLFF, "nsvf": NSVF, "opencv": OpenCV}


def get_dataset(split: str, flags, device=None, rng=np.random, prefetch: int = 3):
    """datasets.py:34-35: the dataset class `flags.dataset` names, loaded onto `device` (None: the current device).  rng and prefetch go
    to the train split's DeviceBatcher."""
    return dataset_dict[flags.dataset](split, flags, device=device, rng=rng, prefetch=prefetch)


def load_masks(data_dir: str, split: str, flags, device=None) -> torch.Tensor:
    """The mask_<name>.png beside each frame of the split (mesh_mask.mask_file_name; metric/summary.py:134-143 reads the same paths) as
    uint8 [n, h, w] on the device, for evaluate.evaluate(masks=...).  Frames as the loader takes them (eval_train, skip_frames); the first
    channel of a colour mask (summary.py:178-180).  With factor 2 every second row and column, m[:, ::2, ::2]: cv2.INTER_NEAREST at an
    exact halving (summary.py:187)."""
    from types import SimpleNamespace
    from . import mesh_mask
    if flags.dataset not in ("blender", "opencv"):
        raise ValueError(f"load_masks: mask files are defined beside the frames of the 'blender' and 'opencv' datasets, not {flags.dataset!r}")
    scoped = SimpleNamespace(**dict(vars(flags), data_dir=data_dir))
    index = INDEXERS[flags.dataset](split, scoped)
    from PIL import Image
    masks = []
    for fp in index.frame_paths:
        fname = os.path.join(data_dir, mesh_mask.mask_file_name(fp, flags.dataset))
        with open(fname, "rb") as f:
            m = np.asarray(Image.open(f))
        if m.ndim == 3:
            m = m[..., 0]
        if m.dtype != np.uint8 or m.ndim != 2:
            raise ValueError(f"{fname}: need an 8-bit mask, got {m.dtype} {m.shape}")
        masks.append(m)
    if not masks:
        raise ValueError("load_masks: the split has no frames")
    if any(m.shape != masks[0].shape for m in masks):
        raise ValueError("load_masks: the masks of a scene must have one size")
    m = torch.from_numpy(np.stack(masks, axis=0)).to(torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return m[:, ::2, ::2].contiguous() if index.factor == 2 else m
