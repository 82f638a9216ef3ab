"""metric/compare.py's win/loss frame (:216-236) and metric/export.py's strip (:92-133) restated in numpy (host only), written for this
repository as errmap_ref.py is.  compare.py imports cv2, lpips and imageio at module level and does its work inside main() on
hard-coded paths, so it cannot be run here to make a golden file; tests/test_compare_host.py holds this file to answers derived by
hand instead.  The text labels (put_text) are left out, as on the device."""
import numpy as np

GAP = 5
TIE = 1e-3                                # compare.py:221, a Python float
COLOUR_A, COLOUR_TIE, COLOUR_B = (239, 138, 98), (247, 247, 247), (103, 169, 207)      # compare.py:225-227
CLASS_A, CLASS_TIE, CLASS_B, CLASS_NEITHER = 0, 1, 2, 3


def save_img_bytes(img):
    """save_img (compare.py:40): np.clip(255.0 * img, 0, 255).astype(np.uint8) on a float64 image."""
    return np.clip(255.0 * np.asarray(img, np.float64), 0, 255).astype(np.uint8)


def masks(map1, map2):
    """compare.py:221-223 without the channel axis -> (non, pos, neg), float64 0 / 1 as there."""
    map1, map2 = np.asarray(map1, np.float32), np.asarray(map2, np.float32)
    with np.errstate(invalid="ignore"):
        non = np.abs(map1 - map2) < TIE
        pos = (1 - non) * (map1 <= map2)
        neg = (1 - non) * (map1 > map2)
    return non, pos, neg


def classify(map1, map2):
    """-> int64 [h, w]: CLASS_A where pos, CLASS_TIE where non, CLASS_B where neg, CLASS_NEITHER where none of them (a NaN)."""
    non, pos, neg = masks(map1, map2)
    assert ((non + pos + neg) <= 1).all()
    return np.where(non, CLASS_TIE, np.where(pos == 1, CLASS_A, np.where(neg == 1, CLASS_B, CLASS_NEITHER))).astype(np.int64)


def colours():
    """The bytes of the four classes, uint8 [4, 3], each computed as compare.py:225-228 computes a pixel of that class: the float64
    sum c_A / 255.0 * pos + c_tie / 255.0 * non + c_B / 255.0 * neg, then save_img."""
    rows = []
    for non, pos, neg in ((0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0)):
        im = np.array(COLOUR_A) / 255.0 * pos + np.array(COLOUR_TIE) / 255.0 * non + np.array(COLOUR_B) / 255.0 * neg
        rows.append(save_img_bytes(im))
    return np.stack(rows)


def float_image(map1, map2):
    """compare.py:221-227 -> float64 [h, w, 3], the image `im` there."""
    non, pos, neg = (m[..., None] for m in masks(map1, map2))
    return np.array(COLOUR_A)[None, None] / 255.0 * pos + np.array(COLOUR_TIE)[None, None] / 255.0 * non + \
        np.array(COLOUR_B)[None, None] / 255.0 * neg


def colorize(map1, map2):
    """compare.py:221-228 -> uint8 [h, w, 3]: {name}_NNN.png."""
    return save_img_bytes(float_image(map1, map2))


def counts(maps1, maps2):
    """int64 [K, 4]: the pixels of each map that are {A's, tied, B's, neither's}."""
    return np.array([np.bincount(classify(a, b).ravel(), minlength=4) for a, b in zip(maps1, maps2)], np.int64).reshape(-1, 4)


def frame(maps1, maps2, H, W):
    """compare.py:216-236 -> uint8 [H, K (W + 5), 3]: each map in the top-left corner of an H x W panel of ones, 5 columns of ones
    after every panel, through save_img."""
    merge = []
    for a, b in zip(maps1, maps2):
        im = float_image(a, b)
        pad = np.ones((H, W, 3))
        pad[:im.shape[0], :im.shape[1]] = im
        merge += [pad, np.ones((H, GAP, 3))]
    out = save_img_bytes(np.hstack(merge))
    assert out.shape == (H, len(merge) // 2 * (W + GAP), 3)
    return out


def strip_table():
    """export.py:103-105 at weight 0.5 for every byte value: uint8 [256]."""
    v = np.arange(256, dtype=np.uint8)
    return np.clip(((v / 255.0) * 0.5 + 1.0 * (1 - 0.5)) * 255.0, 0, 255).astype(np.uint8)


def fade(img, rect):
    """export.py:102-105 on one uint8 image; rect = (x, y, w, h)."""
    h, w = img.shape[:2]
    cx, cy, cw, ch = rect
    mask = np.ones((h, w, 3))
    weight = np.ones((h, w, 3)) * 0.5
    weight[cy:(cy + ch), cx:(cx + cw)] = 1.0
    return np.clip(((img / 255.0) * weight + mask * (1 - weight)) * 255.0, 0, 255).astype(np.uint8)


def strip(images, reference, rect=None):
    """export.py:92-133 without the labels and the BGR flip -> uint8 [H, N (W + 5) + W, 3].  rect None, or with w == 0 or h == 0: no
    fading (CROP off)."""
    H = reference.shape[0]
    white = np.ones((H, GAP, 3), dtype=np.uint8) * 255
    parts = []
    for im in images:
        im = np.asarray(im, np.uint8)
        if rect is not None and rect[2] != 0 and rect[3] != 0:
            im = fade(im, rect)
        parts += [im, white]
    return np.hstack(parts + [np.asarray(reference, np.uint8)])
