"""tests/helpers/lazy_table.py, proven before it judges a kernel (no GPU): its rows are R.build_table's of the dense grid bit for bit, and the
oracle's consumers (R.linear3, R.path_sampler) cannot tell the lazy table from the dense one — on the smallest grids (every voxel is an
edge voxel at (2, 2, 2)) and on a non-cubic one, with box extents that differ per axis."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from lazy_table import LazyTable          # noqa: E402
from oracle import ref_np as R          # noqa: E402

F32 = np.float32
NMIN, NMAX = [-1.5, -1.0, -0.5], [1.4, 1.2, 0.9]
DIMS = [(7, 10, 9), (2, 3, 5), (2, 2, 2)]


def make(dims, seed=0):
    """Profiles whose sum leaves [0, 1] on both sides, so that the clip is active in part of the grid."""
    rng = np.random.default_rng(seed)
    return LazyTable(*[rng.uniform(-0.2, 0.6, n).astype(F32) for n in dims], dims, NMIN, NMAX)


@pytest.mark.parametrize("dims", DIMS)
def test_lazy_rows_are_build_table_rows(dims):
    lz = make(dims)
    grid = lz.dense_grid()
    assert grid.dtype == F32 and grid.shape == tuple(dims)
    assert len(np.unique(grid)) > 4
    if grid.size > 100:
        assert float(grid.min()) == 1.0 and float(grid.max()) == 1.5          # both ends of the clip are active somewhere
    dense = R.build_table(grid, list(dims), NMIN, NMAX)
    flat = np.arange(dense.shape[0])
    rows = lz[flat]
    assert rows.dtype == F32 and rows.shape == dense.shape == lz.shape
    np.testing.assert_array_equal(rows.view(np.uint32), dense.view(np.uint32))
    # any index shape, any integer type, repeated indices
    pick = np.random.default_rng(1).integers(0, dense.shape[0], (5, 3)).astype(np.int32)
    np.testing.assert_array_equal(lz[pick].view(np.uint32), dense[pick].view(np.uint32))
    assert float(np.abs(dense[:, 1:]).max()) > 0
    # the torch face: the same rows as float64 / float32
    torch = pytest.importorskip("torch")
    t64 = lz.torch_face()
    got = t64[torch.from_numpy(pick.astype(np.int64))]
    assert got.dtype == torch.float64 and torch.equal(got, torch.from_numpy(dense[pick]).double())
    got32 = t64.float()[torch.from_numpy(pick.astype(np.int64))]
    assert got32.dtype == torch.float32 and torch.equal(got32, torch.from_numpy(dense[pick]))


@pytest.mark.parametrize("dims", DIMS)
def test_oracle_consumers_cannot_tell_lazy_from_dense(dims):
    lz = make(dims, seed=2)
    dense = R.build_table(lz.dense_grid(), list(dims), NMIN, NMAX)
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1.9, 1.9, (500, 3)).astype(F32)                 # inside and outside the box (clamp-to-edge)
    pts[:2] = [NMIN, NMAX]
    a, ia = R.linear3(lz, pts, list(dims), NMIN, NMAX, return_idx=True)
    b, ib = R.linear3(dense, pts, list(dims), NMIN, NMAX, return_idx=True)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    o = (4.0 * R.safe_l2_normalize(rng.standard_normal((40, 3)).astype(F32))).astype(F32)
    d = R.safe_l2_normalize((rng.uniform(NMIN, NMAX, (40, 3)) - o).astype(F32))
    got = R.path_sampler(o, d, lz, list(dims), NMIN, NMAX, 2.0, 6.0, 48, return_idx=True)
    want = R.path_sampler(o, d, dense, list(dims), NMIN, NMAX, 2.0, 6.0, 48, return_idx=True)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == F32 else g, w.view(np.uint32) if w.dtype == F32 else w)
    assert float(np.abs(want[4]).max()) > 0                           # the rays do meet a gradient
