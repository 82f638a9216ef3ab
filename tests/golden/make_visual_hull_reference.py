"""Golden vectors computed BY THE REFERENCE's own visual-hull text: calib/make_visual_hull.py.

The module cannot be imported here (it imports cv2, trimesh and mcubes), but the three functions the carving needs use numpy only.  This
script reads the FunctionDefs to_view_matrix, project_2d and create_init_bounding_box out of the reference's source with `ast` (nothing
is imported from the reference, nothing of it is copied into this repository), refuses decorated definitions, takes the file's sha256
before anything is compiled, and runs them with numpy as `np` and a whitelist of builtins.  main()'s loop (:107-141) cannot be taken the
same way — it reads calib.json, cfg and image files — so it is restated around them, statement for statement, with arrays standing in for
cv2.imread(mask_fname)[..., 0].

Three cases, the smallest at which each thing can go wrong:
  A "orbit"    G = 24, 8 cameras on an orbit outside the box, 48 x 64 masks; one view looks past the object so that its mask touches the
               image border and clipping to the edge pixel decides voxels.
  B "default"  G = 21 (partial bricks), 6 cameras, the box of create_init_bounding_box: the cameras are inside the grid and c <= 0
               occurs; 40 x 72 masks (a width that is no multiple of 32).
  C "many"     G = 12, 70 views of 16 x 20 masks: more views than a 64-bit word of flags, more than one chunk.

Conditions on the inputs (asserted here, the measured minima stored; they are not tolerances): over every voxel-view pair whose u lies in
[-1, W] and v in [-1, H], the distance of u and of v to the nearest half-integer is above 1e-6 px and |c| is above 1e-6.  Pairs outside
that window clip to the same edge pixel whatever the rounding.  Two float64 evaluation orders of the projection differ by about 4e-14 px
on these inputs (measured below and stored as order_diff_<case>), so the counts do not depend on summation order or FMA use and the tests
demand exact equality with no voxel excluded.  Each case has a non-trivial answer: at threshold 0.9 the hull is neither empty nor full,
at least five distinct count values occur, in A a clipped pixel is inside for some voxel, in B some voxel has c <= 0 in some view.

Inputs, count, data, the boxes, the minima and the source's sha256 go to tests/golden/visual_hull_reference.npz — data, not source.

usage: python tests/golden/make_visual_hull_reference.py [out.npz] | --check"""
import ast
import hashlib
import os
import sys

import numpy as np

REF = os.environ.get("RNERF_REFERENCE_ROOT", "/root/reference")
SRC = os.path.join(REF, "calib", "make_visual_hull.py")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "visual_hull_reference.npz")

NEEDED = ("to_view_matrix", "project_2d", "create_init_bounding_box")
CASES = ("A", "B", "C")
THRESHOLD = 0.9                                          # calib/cfg.py:16
MIN_HALF_DIST = 1e-6
MIN_ABS_C = 1e-6
# name: G, views, H, W, (fx, fy, cx, cy), orbit radius, object radius, default box, seed
SPEC = {"A": dict(G=24, V=8, H=48, W=64, intr=(61.3, 60.7, 31.7, 23.4), orbit=3.1, obj=0.55, default_box=False, seed=5),
        "B": dict(G=21, V=6, H=40, W=72, intr=(47.9, 48.6, 35.6, 20.3), orbit=1.0, obj=0.3, default_box=True, seed=2),
        "C": dict(G=12, V=70, H=16, W=20, intr=(19.3, 18.9, 9.7, 8.2), orbit=3.4, obj=0.6, default_box=False, seed=1)}

_b = __builtins__ if isinstance(__builtins__, dict) else vars(__builtins__)
SAFE_BUILTINS = {k: _b[k] for k in ("range", "len", "int", "float", "list", "tuple", "min", "max", "abs")}


def _numpy_only_import(name, *args, **kwargs):
    """numpy imports its own submodules lazily through the calling frame's builtins: allow exactly that."""
    if name.split(".")[0] != "numpy":
        raise ImportError(f"the visual-hull functions may import numpy only, not {name!r}")
    import builtins
    return builtins.__import__(name, *args, **kwargs)


SAFE_BUILTINS["__import__"] = _numpy_only_import


def source_sha256():
    return hashlib.sha256(open(SRC, "rb").read()).hexdigest() if os.path.exists(SRC) else None


def reference_functions(expect_sha256=None):
    """({name: function} compiled from the reference's text, the file's sha256); (None, None) when the reference is not on this machine.
    The hash is taken BEFORE anything of the file is compiled; with `expect_sha256` a file that is not the one the fixture was made from
    is refused unexecuted."""
    if not os.path.exists(SRC):
        return None, None
    raw = open(SRC, "rb").read()
    sha = hashlib.sha256(raw).hexdigest()
    if expect_sha256 is not None and sha != expect_sha256:
        raise RuntimeError(f"{SRC}: sha256 {sha[:16]} is not the source the committed vectors were made from ({expect_sha256[:16]}): "
                           "nothing of it was executed; re-run tests/golden/make_visual_hull_reference.py after reading the diff")
    tree = ast.parse(raw.decode(), SRC)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NEEDED]
    if sorted(f.name for f in fns) != sorted(NEEDED):
        raise RuntimeError(f"{SRC}: expected exactly one definition of each of {NEEDED}")
    if any(f.decorator_list for f in fns):
        raise RuntimeError(f"{SRC}: a function the carving needs carries a decorator: refusing to execute it")
    ns = {"__builtins__": dict(SAFE_BUILTINS), "np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), SRC, "exec"), ns)
    return {k: ns[k] for k in NEEDED}, sha


def look_at(pos, target):
    """Camera-to-world 4 x 4 (OpenCV axes: x right, y down, z forward) of a camera at `pos` looking at `target`, world z up."""
    f = target - pos
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.array([0.0, 0.0, 1.0]))
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = r, d, f, pos
    return T


def case_inputs(name):
    """-> dict(cam_mat [3,3], transforms [V,4,4], masks uint8 [V,H,W] in {0, 255}, G, box (min, max) or None).  The object is a ball at
    `centre`; each mask is the disc of its silhouette (centre projected, radius f * R / depth), cut by the image."""
    s = SPEC[name]
    rng = np.random.default_rng(20261017 + 1000 * (ord(name) - ord("A")) + s["seed"])
    fx, fy, cx, cy = s["intr"]
    cam_mat = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    V, H, W = s["V"], s["H"], s["W"]
    centre = rng.uniform(-0.08, 0.08, 3) * (s["orbit"] / 3.0)
    transforms, masks = [], []
    for v in range(V):
        az = 2 * np.pi * (v + rng.uniform(-0.2, 0.2)) / V * (3 if name == "C" else 1)
        el = rng.uniform(-0.5, 0.6)
        pos = s["orbit"] * rng.uniform(0.9, 1.1) * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        target = centre + rng.uniform(-0.05, 0.05, 3) * s["orbit"] / 3.0
        if name == "A" and v == 0:                       # looks past the object: its silhouette is cut by the image border
            target = centre + 0.36 * s["orbit"] * look_at(pos, centre)[:3, 0]
        T = look_at(pos, target)
        transforms.append(T)
        pc = T[:3, :3].T @ (centre - pos)                # the object's centre in camera axes
        u0, v0, rad = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy, 0.5 * (fx + fy) * s["obj"] / pc[2]
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        masks.append(((xx - u0) ** 2 + (yy - v0) ** 2 <= rad ** 2).astype(np.uint8) * 255)
    box = None if s["default_box"] else (np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0]))
    return dict(cam_mat=cam_mat, transforms=np.stack(transforms), masks=np.stack(masks), G=s["G"], box=box)


def run_reference(fns, x, threshold=THRESHOLD):
    """make_visual_hull.py:92-141 around the reference's functions.  -> dict(count int32 [G,G,G], data float64 [G^3,1], min_point,
    max_point, view_mats, and the measured conditions)."""
    to_view_matrix, project_2d, create_init_bounding_box = (fns[k] for k in NEEDED)
    cam_mat = np.array(x["cam_mat"])
    p_mat = np.concatenate([cam_mat, np.zeros((3, 1))], axis=1)
    trans_mats = [np.array(t) for t in x["transforms"]]
    view_mats = [to_view_matrix(np.array(t)) for t in x["transforms"]]
    mask_imgs = list(x["masks"])
    num_imgs = len(mask_imgs)
    num_voxels = x["G"]
    if x["box"] is None:
        max_point, min_point = create_init_bounding_box(trans_mats)
    else:
        max_point, min_point = x["box"][1], x["box"][0]
    Y, X, Z = np.meshgrid(np.linspace(0, 1, num_voxels), np.linspace(0, 1, num_voxels), np.linspace(0, 1, num_voxels))
    x_max, y_max, z_max = max_point
    x_min, y_min, z_min = min_point
    X = X * (x_max - x_min) + x_min
    Y = Y * (y_max - y_min) + y_min
    Z = Z * (z_max - z_min) + z_min
    pts = np.concatenate([np.stack([X, Y, Z], axis=-1), np.ones((num_voxels, num_voxels, num_voxels, 1))], axis=-1)
    count = np.zeros((num_voxels, num_voxels, num_voxels))
    half, absc, neg_c, clipped_inside, order = np.inf, np.inf, 0, 0, 0.0
    for view_mat, mask_img in zip(view_mats, mask_imgs):
        uvs, zs = project_2d(pts, p_mat, view_mat)
        us = np.clip(np.round(uvs[..., 0]), 0, mask_img.shape[1] - 1).astype(int)
        vs = np.clip(np.round(uvs[..., 1]), 0, mask_img.shape[0] - 1).astype(int)
        inside = mask_img[vs.reshape(-1), us.reshape(-1)] > 0
        inside = inside.reshape(num_voxels, num_voxels, num_voxels)
        count += inside
        # the conditions, measured on the reference's own u, v, c (uvs[..., 2] is c: project_2d divides the first two columns only)
        u, v, c = uvs[..., 0], uvs[..., 1], uvs[..., 2]
        H, W = mask_img.shape
        win = (u >= -1) & (u <= W) & (v >= -1) & (v <= H)
        for a in (u[win], v[win]):
            if a.size:
                half = min(half, float(np.min(np.abs(a - np.floor(a) - 0.5))))
        if win.any():
            absc = min(absc, float(np.min(np.abs(c[win]))))
        neg_c += int(np.sum(c <= 0))
        clipped_inside += int(np.sum(inside & ((np.round(u) < 0) | (np.round(u) > W - 1) | (np.round(v) < 0) | (np.round(v) > H - 1))))
        # a second evaluation order of the same projection (right to left), for the record
        pv = p_mat @ view_mat
        alt = [pv[r, 3] + (pts[..., 2] * pv[r, 2] + (pts[..., 1] * pv[r, 1] + pts[..., 0] * pv[r, 0])) for r in range(3)]
        with np.errstate(divide="ignore", invalid="ignore"):
            du, dv = np.abs(alt[0] / alt[2] - u), np.abs(alt[1] / alt[2] - v)
        if win.any():
            order = max(order, float(np.max(du[win])), float(np.max(dv[win])))
    counts = count.astype(np.int32)
    count /= num_imgs
    data = (count > threshold).reshape(-1, 1) * 0.33 + 1.0
    return dict(count=counts, data=data, min_point=np.asarray(min_point, np.float64), max_point=np.asarray(max_point, np.float64),
                view_mats=np.stack(view_mats), min_half_dist=half, min_abs_c=absc, num_c_le_0=neg_c, num_clipped_inside=clipped_inside,
                order_diff=order)


def assert_conditions(name, x, r):
    hull = r["data"] > 1.0
    assert r["min_half_dist"] > MIN_HALF_DIST, f"{name}: a projection lies {r['min_half_dist']:.3g} px from a rounding boundary: change the seed"
    assert r["min_abs_c"] > MIN_ABS_C, f"{name}: |c| = {r['min_abs_c']:.3g} inside the window: change the seed"
    assert r["order_diff"] < 1e-9, f"{name}: two evaluation orders differ by {r['order_diff']:.3g} px"
    assert 0 < hull.sum() < hull.size, f"{name}: the hull is empty or full"
    assert len(np.unique(r["count"])) >= 5, f"{name}: fewer than five distinct counts"
    m = x["masks"]
    if name == "A":
        assert any((mm[0] > 0).any() or (mm[-1] > 0).any() or (mm[:, 0] > 0).any() or (mm[:, -1] > 0).any() for mm in m), "A: no mask touches the border"
        assert r["num_clipped_inside"] > 0, "A: clipping decides no voxel"
    if name == "B":
        assert r["num_c_le_0"] > 0, "B: no voxel with c <= 0"
        assert m.shape[2] % 32 != 0


def compute(fns):
    res = {}
    for name in CASES:
        x = case_inputs(name)
        r = run_reference(fns, x)
        assert_conditions(name, x, r)
        res[name] = (x, r)
    return res


STORED = ("count", "data", "min_point", "max_point", "view_mats", "min_half_dist", "min_abs_c", "num_c_le_0", "num_clipped_inside", "order_diff")


def main(path=OUT):
    fns, sha = reference_functions()
    if fns is None:
        print(f"SKIPPED: {SRC} is not on this machine")
        return None
    arrays = {"source_sha256": np.array(sha), "threshold": np.float64(THRESHOLD)}
    for name, (x, r) in compute(fns).items():
        arrays[f"{name}_cam_mat"], arrays[f"{name}_transforms"], arrays[f"{name}_masks"] = x["cam_mat"], x["transforms"], x["masks"]
        arrays[f"{name}_G"] = np.int32(x["G"])
        arrays[f"{name}_default_box"] = np.bool_(x["box"] is None)
        for k in STORED:
            arrays[f"{name}_{k}"] = np.asarray(r[k])
        print(f"{name}: G {x['G']}, {len(x['masks'])} views, hull {int((r['data'] > 1).sum())} of {r['data'].size} voxels, "
              f"{len(np.unique(r['count']))} distinct counts, min half-integer distance {r['min_half_dist']:.3g} px, min |c| {r['min_abs_c']:.3g}, "
              f"c <= 0: {r['num_c_le_0']}, clipped and inside: {r['num_clipped_inside']}, order difference {r['order_diff']:.3g} px")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(CASES)} cases computed by {SRC} (sha256 {sha[:16]}), {os.path.getsize(path)} bytes")
    return path


def load_case(d, name):
    """The inputs of a case as stored in the file (a mapping from np.load)."""
    box = None if bool(d[f"{name}_default_box"]) else (d[f"{name}_min_point"], d[f"{name}_max_point"])
    return dict(cam_mat=d[f"{name}_cam_mat"], transforms=d[f"{name}_transforms"], masks=d[f"{name}_masks"], G=int(d[f"{name}_G"]), box=box)


def check(path=OUT):
    """`--check`: the committed vectors are what the reference computes today — same source hash, same bits."""
    if source_sha256() is None:
        raise SystemExit(f"{SRC} is not on this machine: nothing to check against")
    d = np.load(path)
    fns, _ = reference_functions(expect_sha256=str(d["source_sha256"]))
    bad = []
    for name, (x, r) in compute(fns).items():
        bad += [f"{name}_{k}" for k in ("cam_mat", "transforms", "masks") if not np.array_equal(x[k], d[f"{name}_{k}"])]
        bad += [f"{name}_{k}" for k in STORED if not np.array_equal(np.asarray(r[k]), d[f"{name}_{k}"])]
    print(f"{path}: " + ("equals what the reference computes, bit for bit" if not bad else "DIFFERS in " + ", ".join(bad)))
    return not bad


if __name__ == "__main__":
    if sys.argv[1:] == ["--check"]:
        raise SystemExit(0 if check() else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
