#!/usr/bin/env python3
"""Fixture generator (needs the reference's example data): a window of the one real training view, as the PNG holds it.

    python tests/golden/make_example_scene.py        ->  tests/golden/example_scene.npz

Reads example_data/imgs/r_0.png (800 x 800 RGBA) and example_data/transforms_train.json of the reference and stores
  window             uint8 [64, 96, 4]: rows origin[0] .. +64, columns origin[1] .. +96 of the decoded image, untouched
  origin             (row, column) of the window, both even — the window is whole 2 x 2 cells of tests/golden/example_image.npz's `rgba_sum4`
  camera_angle_x, transform_matrix   of the frame
The image is rendered against a sky dome: its alpha channel is 255 in every pixel, so there is no alpha edge to put the window on (partial
alpha is covered by the synthetic scenes of tests/helpers/scene_fixture.py).  The window is instead the one with the largest spread of
luminance among the even origins on a 32-pixel lattice: the object's outline against the background.  tests/test_scene_loader_host.py and tests/test_gpu_scene_loader.py
write a one-frame Blender scene from it and load it with `factor: 2`.  Pixels and numbers only — no text of any reference source."""
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNERF_REFERENCE_ROOT", "/root/reference")
WH, WW = 64, 96


def main():
    im = np.array(Image.open(os.path.join(REF, "example_data", "imgs", "r_0.png")))
    assert im.shape == (800, 800, 4) and im.dtype == np.uint8, (im.shape, im.dtype)
    with open(os.path.join(REF, "example_data", "transforms_train.json")) as fp:
        meta = json.load(fp)
    frame = meta["frames"][0]
    assert frame["file_path"].endswith("r_0"), frame["file_path"]
    best = None
    for r in range(0, 800 - WH + 1, 32):
        for c in range(0, 800 - WW + 1, 32):
            score = -float(im[r:r + WH, c:c + WW, :3].astype(np.float64).sum(-1).std())
            if best is None or score < best[0]:
                best = (score, r, c)
    _, r, c = best
    out = os.path.join(HERE, "example_scene.npz")
    np.savez_compressed(out, window=im[r:r + WH, c:c + WW], origin=np.array([r, c]), camera_angle_x=np.array(float(meta["camera_angle_x"])),
                        transform_matrix=np.array(frame["transform_matrix"], np.float64))
    print(out, os.path.getsize(out), "bytes; origin", (r, c), "luminance spread", -best[0], "alpha", np.unique(im[..., 3]))


if __name__ == "__main__":
    main()
