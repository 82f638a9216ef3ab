"""Marching cubes without a GPU: the generated case table, the C ABI's argument checks, the OBJ writer, the preview transforms and the
numpy oracle (tests/helpers/marching_cubes_ref.py) on the example scene's grid.

The table proof: for every case and face, the directed triangle edges that lie in the face and have no partner inside the cell depend
only on that face's four corner bits and are the reverse of what the cell on the other side leaves there.  With that, the surface of
ANY field is closed and consistently oriented wherever it does not leave the grid.

The reference ships one marching-cubes mesh, example_data/voxelize/mesh_4_128_1.5_1.165.obj (tests/golden/example_obj.npz).  PyMCubes'
vertex order and triangulation are not reproduced, so the comparison is of what is pinned: a closed oriented 2-manifold with
V - E + F = 2, vertices on grid edges, signed volume +311 331.7 index units^3.  The oracle on the re-voxelised grid (not the original
one): 27 624 vertices, 55 244 triangles, volume +310 912.1, 0.13 % apart; asserted: the sign and 1 %."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import marching_cubes_ref as MR             # noqa: E402

NEW_SYMBOLS = ("rnerf_marching_cubes_workspace_bytes", "rnerf_marching_cubes_count", "rnerf_marching_cubes_emit", "rnerf_marching_cubes_table")


@pytest.fixture(scope="module")
def table(lib_path):
    from samplenerfro_amd import marching_cubes
    t = marching_cubes.case_table()
    t.setflags(write=False)
    return t


def rows(table, case):
    r = table[case]
    n = int((r >= 0).sum())
    assert n % 3 == 0 and np.all(r[n:] == -1)
    return [tuple(int(v) for v in r[i:i + 3]) for i in range(0, n, 3)]


def test_new_symbols_are_declared_bound_and_exported(lib_path):
    from samplenerfro_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rnerf.h")).read()
    lib = ctypes.CDLL(lib_path)
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.load().rnerf_version() == 4                                  # appended: the ABI version does not move
    for site in ("voxelize_mesh.py:122-135", "make_visual_hull.py:148-157", "extract_mesh.py:232-268"):
        assert site in hdr
    import samplenerfro_amd
    assert samplenerfro_amd.marching_cubes.marching_cubes is not None and samplenerfro_amd.extract.extract_mesh is not None


def test_table_equals_the_one_derived_from_the_face_rule(table):
    want, ntri = MR.table()
    assert table.shape == (256, 16) and table.dtype == np.int8
    bad = np.nonzero((table != want).any(1))[0]
    assert len(bad) == 0, f"cases {bad.tolist()} differ"


def test_committed_header_is_the_generators_output():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_mc_tables
    assert open(os.path.join(ROOT, "samplenerfro_amd", "csrc", "mc_tables.h")).read() == make_mc_tables.render()


def test_counts(table):
    n = np.array([len(rows(table, c)) for c in range(256)])
    assert n[0] == 0 and n[255] == 0 and n.max() == 5 and n.sum() == 820
    assert np.bincount(n, minlength=6).tolist() == [2, 16, 50, 80, 76, 32]


def test_every_triangle_uses_distinct_active_edges_and_every_active_edge_is_used(table):
    for case in range(256):
        active = {e for e in range(12) if MR.bit(case, MR.edge_ends(e)[0]) != MR.bit(case, MR.edge_ends(e)[1])}
        used = set()
        for t in rows(table, case):
            assert len(set(t)) == 3 and set(t) <= active, (case, t)
            used |= set(t)
        assert used == active, case


def in_plane_name(e, d):
    """An edge on a face of axis d, named without its coordinate on d: the same name on both sides of the face."""
    c0, c1 = MR.edge_ends(e)
    drop = lambda c: tuple(v for a, v in enumerate(c) if a != d)
    return (drop(c0), drop(c1))


def test_faces_of_neighbouring_cells_match(table):
    """The proof of closed, oriented output for every input (module docstring)."""
    left = {}                  # (d, side, the face's four bits) -> the set of open directed edges in the face, in-plane names
    for case in range(256):
        directed = [(t[i], t[(i + 1) % 3]) for t in rows(table, case) for i in range(3)]
        assert len(set(directed)) == len(directed), case                     # no directed edge twice
        open_edges = [(u, v) for u, v in directed if (v, u) not in directed]
        per_face = {(d, side): set() for d in range(3) for side in (0, 1)}
        for u, v in open_edges:
            faces = [(d, side) for d in range(3) for side in (0, 1)
                     if all(c[d] == side for c in MR.edge_ends(u) + MR.edge_ends(v))]
            assert len(faces) == 1, (case, u, v)                             # an open edge lies in exactly one face
            d, side = faces[0]
            per_face[(d, side)].add((in_plane_name(u, d), in_plane_name(v, d)))
        for (d, side), got in per_face.items():
            bits = tuple(MR.bit(case, c) for c in MR.face_cycle(d, side))
            crossings = sum(bits[i] != bits[(i + 1) % 4] for i in range(4))
            assert len(got) == crossings // 2, (case, d, side)
            assert left.setdefault((d, side, bits), got) == got, (case, d, side)     # depends on the face's four bits only
    assert len(left) == 6 * 16
    for (d, side, bits), got in left.items():
        other = left[(d, 1 - side, bits)]                                    # the neighbour sees the same bits on its opposite face
        assert {(v, u) for u, v in got} == other, (d, side, bits)


def test_argument_errors_do_not_need_a_gpu(lib_path):
    from samplenerfro_amd import _lib
    lib = _lib.load()
    p, mis = ctypes.c_void_p(256), ctypes.c_void_p(260)
    err = lambda: lib.rnerf_last_error()
    D = lambda *d: ctypes.byref((ctypes.c_int32 * 3)(*d))
    ok = D(8, 8, 8)
    count = lambda field=p, dims=ok, iso=0.5, ws=p, totals=p: lib.rnerf_marching_cubes_count(field, dims, iso, ws, totals, None)
    emit = lambda field=p, dims=ok, iso=0.5, ws=p, verts=p, vc=10, faces=p, fc=10, ovf=p: lib.rnerf_marching_cubes_emit(
        field, dims, iso, ws, verts, vc, faces, fc, ovf, None)

    # null pointers
    assert count(field=None) == -1 and b"null pointer" in err()
    assert count(dims=None) == -1 and b"null pointer" in err()
    assert count(ws=None) == -1 and b"null pointer" in err()
    assert count(totals=None) == -1 and b"null pointer" in err()
    assert emit(field=None) == -1 and b"null pointer" in err()
    assert emit(dims=None) == -1 and emit(ws=None) == -1 and emit(ovf=None) == -1
    assert emit(verts=None) == -1 and b"null pointer" in err()               # with a capacity above 0
    assert emit(faces=None) == -1 and b"null pointer" in err()
    assert lib.rnerf_marching_cubes_table(None) == -1 and b"null pointer" in err()
    assert lib.rnerf_marching_cubes_workspace_bytes(None) == 0 and b"dims" in err()

    # a dim of 1 (or below)
    for d in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (8, -3, 8)):
        assert lib.rnerf_marching_cubes_workspace_bytes(D(*d)) == 0 and b"dims >= 2" in err()
        assert count(dims=D(*d)) == -1 and b"dims >= 2" in err()
        assert emit(dims=D(*d)) == -1 and b"dims >= 2" in err()

    # the size limit 3 N <= 2^31 - 1: vertex indices fit int32
    n894 = 894 ** 3
    assert 3 * n894 <= 2 ** 31 - 1 < 3 * 895 ** 3
    assert lib.rnerf_marching_cubes_workspace_bytes(D(894, 894, 894)) == 8 * ((n894 + 1023) // 1024) + 4 * n894
    assert lib.rnerf_marching_cubes_workspace_bytes(D(895, 895, 895)) == 0 and b"2^31 - 1" in err()
    assert count(dims=D(895, 895, 895)) == -1 and b"2^31 - 1" in err()
    assert emit(dims=D(895, 895, 895)) == -1 and b"2^31 - 1" in err()
    assert count(dims=D(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)) == -1        # no overflow of the product itself
    assert lib.rnerf_marching_cubes_workspace_bytes(D(2, 2, 2)) == 8 + 32
    assert lib.rnerf_marching_cubes_workspace_bytes(D(3, 5, 67)) == 8 + 4 * 1005

    # a non-finite iso
    for iso in (float("nan"), float("inf"), -float("inf")):
        assert count(iso=iso) == -1 and b"finite" in err()
        assert emit(iso=iso) == -1 and b"finite" in err()

    # a misaligned workspace
    assert count(ws=mis) == -1 and b"aligned" in err()
    assert emit(ws=mis) == -1 and b"aligned" in err()

    # negative capacities
    assert emit(vc=-1) == -1 and b"negative capacity" in err()
    assert emit(fc=-1) == -1 and b"negative capacity" in err()


def test_marching_cubes_rejects_a_bad_shape_before_any_device_work(lib_path):
    from samplenerfro_amd import marching_cubes
    with pytest.raises(ValueError):
        marching_cubes.marching_cubes(np.zeros((4, 4), np.float32), 0.5)


def test_save_obj_round_trips_bit_exactly(tmp_path):
    from samplenerfro_amd import marching_cubes, voxelize
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal((200, 3)) * 10.0 ** rng.integers(-12, 12, (200, 1)),
                        [[0.0, -0.0, 1.0], [1 / 3, np.nextafter(1.0, 2.0), 5e-324], [1e308, -1e-308, 0.1]]])
    f = rng.integers(0, len(v), (77, 3)).astype(np.int32)
    path = str(tmp_path / "m.obj")
    marching_cubes.save_obj(path, v, f)
    v2, f2 = voxelize.load_obj(path)
    assert v2.tobytes() == v.tobytes() and np.array_equal(f2, f) and f2.dtype == np.int32
    text = open(path).read().splitlines()
    assert len(text) == len(v) + len(f) and text[0].startswith("v ") and text[-1].startswith("f ")
    assert min(int(t) for line in text[len(v):] for t in line.split()[1:]) >= 1                     # 1-based
    import torch
    marching_cubes.save_obj(path, torch.from_numpy(v), torch.from_numpy(f))                          # tensors are taken too
    v3, f3 = voxelize.load_obj(path)
    assert v3.tobytes() == v.tobytes() and np.array_equal(f3, f)
    marching_cubes.save_obj(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32))                      # an empty mesh is legal
    assert open(path).read() == ""


def test_preview_transforms_agree_with_the_fixtures_world_transform():
    import cases
    from samplenerfro_amd import visual_hull, voxelize
    idx = np.random.default_rng(4).uniform(0, 127, (500, 3))
    idx[:, 0] = np.round(idx[:, 0]); idx[:, 1] = np.round(idx[:, 1])
    obj = voxelize.preview_coords(idx, 128)                                  # what the script writes: vertices / N - 0.5
    assert np.array_equal(obj, idx / 128 - 0.5)
    world = voxelize.world_coords(idx, [128] * 3, [-1.5] * 3, [1.5] * 3)      # sample i at nmin + i / (N - 1) (nmax - nmin)
    assert np.abs(cases.example_obj_world(obj) - world).max() < 1e-13
    assert np.array_equal(voxelize.world_coords(np.array([[0.0, 127.0, 0.0]]), [128] * 3, [-1.5] * 3, [1.5] * 3), [[-1.5, 1.5, -1.5]])
    assert voxelize.preview_name(4, 128, 1.5, 1.165) == "mesh_4_128_1.5_1.165.obj"                  # the file the reference ships
    lo, hi = np.array([-1.0, 0.5, 2.0]), np.array([3.0, 1.5, 2.5])
    got = visual_hull.preview_coords(idx, 128, lo, hi)                       # make_visual_hull.py:151-154
    assert np.array_equal(got, idx / 128 * (hi - lo) + lo)
    import torch
    assert np.array_equal(voxelize.world_coords(torch.from_numpy(idx), [128] * 3, [-1.5] * 3, [1.5] * 3).numpy(), world)
    assert np.array_equal(visual_hull.preview_coords(torch.from_numpy(idx), 128, lo, hi).numpy(), got)
    for N in (24, 100):                                                      # a true division where 1 / N is not exact
        assert np.array_equal(visual_hull.preview_coords(torch.from_numpy(idx), N, lo, hi).numpy(), idx / N * (hi - lo) + lo)
        assert np.array_equal(voxelize.preview_coords(torch.from_numpy(idx), N).numpy(), idx / N - 0.5)


def test_oracle_on_the_example_grid_against_the_shipped_obj():
    import cases
    verts, faces, counts = cases.load_example_obj()
    shipped = (verts + 0.5) * 128                                            # the OBJ holds mcubes vertices / 128 - 0.5
    assert MR.is_closed_oriented(faces) and MR.euler(shipped, faces) == 2
    on_grid = np.abs(shipped - np.round(shipped)) < 1e-9
    assert np.all(on_grid.sum(1) == 2)                                       # vertices on grid edges, sample i at coordinate i
    vol_shipped = MR.signed_volume(shipped, faces)
    assert abs(vol_shipped - 311331.7) < 0.1

    data = cases.R.counts_to_ior(counts.astype(np.int32), 4).reshape(128, 128, 128)
    v, f = MR.marching_cubes(data, 1.165)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert MR.is_closed_oriented(f) and MR.euler(v, f) == 2 and len(v) == MR.num_crossed_edges(data, 1.165)
    assert len(np.unique(f)) == len(v) and np.all(f[:, 0] != f[:, 1]) and np.all(f[:, 1] != f[:, 2]) and np.all(f[:, 0] != f[:, 2])
    assert np.all((v == np.round(v)).sum(1) >= 2) and v.min() >= 0 and v.max() <= 127
    vol = MR.signed_volume(v, f)
    gap = abs(vol - vol_shipped) / vol_shipped
    ties = int((np.asarray(data, np.float64) == 1.165).sum())                # they stop tying once the field is float32, as the device takes it
    print(f"oracle: {len(v)} vertices, {len(f)} triangles, {ties} voxels tie with the iso in float64; volume {vol:.1f} against the shipped "
          f"{vol_shipped:.1f}: {100 * gap:.3f} % apart")
    assert vol > 0 and vol_shipped > 0 and gap < 0.01
