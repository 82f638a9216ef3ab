"""The resampler's test cases on the CPU (tests/helpers/resample_cases.py): the numpy oracle and the scalar C reading of sample_pdf agree
BIT FOR BIT on every depth / weight / u family (front- and back-loaded node depths, runs of equal node depths, dl == d0, planted cdf ties,
a float32 running sum that overshoots 1) — the licence to hold the kernels to the C reading alone where the dense mask of the numpy oracle
is too large — and every case reaches the edge it was built for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_cases as RC                                      # noqa: E402
from oracle import ref_np as R                                   # noqa: E402

F32 = np.float32


def _same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a.view(np.uint32 if a.dtype == F32 else a.dtype), b.view(np.uint32 if b.dtype == F32 else b.dtype))


@pytest.mark.parametrize("name", RC.host_names())
def test_numpy_and_c_readings_agree_and_the_case_reaches_its_edge(name):
    d = RC.build(RC.CASES[name])
    c = d["case"]
    z, p, dr, idx = RC.reference_np(d)
    zc, pc, dc, ic = RC.reference_c(d)
    _same_bits(idx, ic)
    _same_bits(z, zc); _same_bits(p, pc); _same_bits(dr, dc)
    assert z.shape == (c.B, c.S + c.F) and (np.diff(z, axis=1) >= 0).all() and idx.min() >= 0 and idx.max() <= c.S * c.P - 1
    if c.F == 0:                                                  # nothing to merge: the coarse rows themselves
        np.testing.assert_array_equal(idx, np.broadcast_to(np.maximum(_first_node(d) - 1, 0), idx.shape))
        np.testing.assert_array_equal(z, d["z_vals"][:, d["jitter"]])
    RC.check_facts(d, z)


@pytest.mark.parametrize("name", [n for n in RC.names() if n not in RC.host_names()])
def test_large_cases_reach_their_edges(name):
    """The shapes left to the GPU test (one reading there): their input-side facts hold, and their u and depths are well-formed (build asserts)."""
    d = RC.build(RC.CASES[name])
    assert RC.GROUP[name] in ("full_lds", "demoted")
    RC.check_facts(d)


def _first_node(d):
    """searchsorted(z_vals, z_vals[jitter], 'left') per ray."""
    zv, j = d["z_vals"], d["jitter"]
    return np.stack([np.searchsorted(zv[i], zv[i, j], "left") for i in range(zv.shape[0])])


def test_the_table_covers_every_launch_regime_and_family():
    cs = list(RC.CASES.values())
    assert {RC.rays_per_block(c) for c in cs} == {1, 4, 16}
    by = {(RC.need(c), RC.rays_per_block(c)) for c in cs}
    assert {(2560, 16), (10240, 4), (40960, 1)} <= by             # the three launches of exactly 160 KiB
    assert {(2564, 4), (10260, 1), (10416, 1)} <= by              # the demotions
    assert RC.need(RC.REFUSED) == 40962
    for c in cs:
        assert RC.need(c) * RC.rays_per_block(c) * 4 <= 163840
    assert {c.depth for c in cs} == set(RC.DEPTHS) and {c.u for c in cs} == set(RC.US)
    for B in (1025, 8193):                                        # a one-ray tail block
        assert any(c.B == B and c.B % RC.rays_per_block(c) == 1 for c in cs)


def test_overshoot_family_overshoots():
    """Random ** 4 weights whose last three inner weights are zero: the float32 running sum passes 1 on about a quarter of the rays."""
    d = RC.build(RC.CASES["lanes-B8193-S24-P5-F40-linear-overshoot-stratified"])
    assert d["facts"]["overshoot_rays"] >= 82                     # 1 % of 8193
    raw, cdf = RC.cdf_of(d["w"][:, 1:-1])
    assert raw.max() > 1 and cdf.max() == 1 and (np.diff(cdf, axis=1) >= 0).all()


@pytest.mark.parametrize("name", ["lanes-B1025-S12-P5-F40-linear-mixed-ties", "gather-B300-S24-P5-F40-plateau-mixed-ties",
                                  "ragged-B17-S5-P3-F67-linear-mixed-ties"])
def test_a_draw_equal_to_a_cdf_entry_belongs_to_the_interval_that_starts_there(name):
    """u == cdf[k] -> interval k (`cdf <= u`); where zero-width intervals repeat the entry, the last of the equal ones."""
    d = RC.build(RC.CASES[name])
    u, cdf, planted = d["u"], d["cdf"], d["planted"]
    assert len(planted) >= d["case"].B
    _, iv = R.sorted_piecewise_constant_pdf(u, d["bins"], d["w"][:, 1:-1], return_idx=True)
    strict = 0
    for r, k in planted:
        f = np.nonzero(u[r] == cdf[r, k])[0]
        assert len(f) >= 1
        last = int(np.searchsorted(cdf[r], cdf[r, k], "right")) - 1
        assert last >= k and cdf[r, last] == cdf[r, k]
        assert (iv[r, f] == last).all()
        strict += int(last == k)
    assert strict >= d["case"].B // 2                             # mostly plain entries: interval k itself
