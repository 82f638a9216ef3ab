"""rnerf_resample (resample_depths_kernel<16|4|1> + resample_gather_kernel) against the oracle, BIT FOR BIT, in every launch regime of the
product launcher and at its edges (tests/helpers/resample_cases.py has the table):

  * both sides of each composite_lanes threshold, with the one-ray tail blocks of 1025 = 4 * 256 + 1 and 8193 = 16 * 512 + 1 rays;
  * ragged and minimal shapes (one weight, F = 0 / 1 / 2, S below every lane count);
  * the largest launch of each instantiation (exactly 160 KiB of dynamic LDS), the two LDS demotions and the refusal beyond 40960 floats;
  * node depths on which the gather's arithmetic guess is far off in either direction, runs of equal node depths, dl == d0;
  * draws that equal cdf entries, zero-width cdf intervals, the padding branch and a float32 running sum that overshoots 1.

Node index, merged depth, position and direction involve + - * / only, individually rounded: assert_array_equal, no tolerance.  The
comparison is taken on the device (torch.equal against the uploaded reference: the largest case holds about 0.7 GB of rows) and restated
with numpy only to report a mismatch.  The reference is oracle.ref_np.sample_pdf chunked over rays, or the scalar C reading (held to the
numpy one bit for bit by tests/test_resample_cases_host.py) where the dense mask is too large; a C reading that cannot be built fails.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_cases as RC                                      # noqa: E402
from samplenerfro_amd import _lib                                # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no ROCm device is visible")
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _assert_same(got, want, what):
    """got: device tensor, want: numpy array of the same shape."""
    assert tuple(got.shape) == want.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), want.shape)
    if bool(torch.equal(got, T(want))):
        return
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=what)
    pytest.fail("%s: differs from the reference (NaN against NaN)" % what)


def _run(d, want_idx=True):
    from samplenerfro_amd import ops
    return ops.resample(T(d["path_pd"]), T(d["path_dr"]), T(d["jitter"]), T(d["w_t"]), T(d["u_dev"]), d["case"].F, want_idx=want_idx)


@pytest.mark.parametrize("name", RC.names())
def test_resample_bit_exact(name):
    c = RC.CASES[name]
    d = RC.build(c)
    ref = RC.reference(d)
    RC.check_facts(d, ref[0])
    want_pd, want_dr, want_idx = RC.device_rows(ref)
    del ref
    rows_pd, rows_dr, idx = _run(d)
    _assert_same(idx, want_idx, "node index")                     # searchsorted node index
    _assert_same(rows_pd[..., 3], want_pd[..., 3], "merged depth")
    _assert_same(rows_pd, want_pd, "position")
    _assert_same(rows_dr, want_dr, "direction")
    if c.F == 0:                                                  # the coarse rows themselves
        j = d["jitter"]
        np.testing.assert_array_equal(rows_pd[..., 3].cpu().numpy(), d["path_pd"][j][..., 3])
        np.testing.assert_array_equal(rows_dr.cpu().numpy(), d["path_dr"][np.maximum(want_idx, 0), np.arange(c.B)[None, :]])


@pytest.mark.parametrize("name", ["lanes-B1024-S12-P5-F40-linear-mixed-ties", "lanes-B1025-S12-P5-F40-linear-mixed-ties",
                                  "lanes-B8193-S12-P5-F40-linear-mixed-ties", "gather-B1025-S24-P5-F40-plateau-mixed-ties",
                                  "ragged-B17-S3-P1-F0-linear-mixed-stratified"])
def test_rows_do_not_depend_on_the_index_output(name):
    """node_idx = nullptr (what the forward passes) against node_idx given: the same rows, one case per instantiation."""
    d = RC.build(RC.CASES[name])
    pd1, dr1, idx = _run(d, want_idx=True)
    pd0, dr0, none = _run(d, want_idx=False)
    assert none is None and idx is not None
    assert bool(torch.equal(pd0, pd1)) and bool(torch.equal(dr0, dr1))


def test_staging_beyond_the_lds_is_refused_and_writes_nothing():
    """need = 4 * 3 + 2 * 20475 = 40962 floats > 40960: RNERF_ERR_ARG with the LDS message, before any device work."""
    c = RC.REFUSED
    assert RC.need(c) == 40962
    d = RC.build(c)
    lib = _lib.load()
    Tn, B, N = c.S + c.F, c.B, c.S * c.P
    pd, dr, jit, w, u = T(d["path_pd"]), T(d["path_dr"]), T(d["jitter"]), T(d["w_t"]), T(d["u_dev"])
    rows_pd = torch.full((Tn, B, 4), -7.0, dtype=torch.float32, device=dev())
    rows_dr = torch.full((Tn, B, 4), -7.0, dtype=torch.float32, device=dev())
    idx = torch.full((Tn, B), -7, dtype=torch.int32, device=dev())
    scratch = torch.full((Tn, B), -7.0, dtype=torch.float32, device=dev())
    rc = lib.rnerf_resample(_lib.ptr(pd), _lib.ptr(dr), N, B, _lib.ptr(jit), c.S, _lib.ptr(w), _lib.ptr(u), 0, c.F, _lib.ptr(rows_pd),
                            _lib.ptr(rows_dr), _lib.ptr(idx), _lib.ptr(scratch), _lib.current_stream())
    msg = lib.rnerf_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1, (rc, msg)                                    # RNERF_ERR_ARG
    assert "LDS" in msg and "40960" in msg, msg
    for t in (rows_pd, rows_dr, scratch):
        assert bool((t == -7.0).all())
    assert bool((idx == -7).all())
    # the same through the Python wrapper: an error, never a quiet result
    from samplenerfro_amd import ops
    with pytest.raises(_lib.RnerfError, match="LDS"):
        ops.resample(pd, dr, jit, w, u, c.F, want_idx=True)
    # one fine sample fewer is the largest launch there is, and it runs
    assert RC.need(RC.CASES["full_lds-B2-S3-P1-F20474-linear-mixed-stratified"]) == 40960
