"""CPU check of the references and bounds that tests/test_vector_gpu.py holds the device to: a NumPy float64 emulation of
the two-stage summation order that the launch constants imply (a thread's trips in order, a fixed tree over the 256
threads of a workgroup, then the partials) runs on the same generators and lengths (up to 524 289 to stay fast) and must
stay inside the stated bounds against the math.fsum and np.longdouble references, and reproduce the integer vectors
exactly.  A correct kernel therefore passes, and the bounds do not hide a failure of the reference itself."""
import math

import numpy as np
import pytest

import vector_refs as vr            # (tests/vector_refs.py)

HOST_NMAX = 524289


def test_longdouble_is_wider_than_double():
    """the scaled-rms reference needs more than double precision to be a reference at all"""
    assert np.finfo(np.longdouble).nmant >= 63


def test_grids_change_where_the_lengths_say():
    """nb, stride and trips from the launch constants: the tested lengths sit on both sides of every change"""
    assert vr.dot_grid(512, False) == (1, 256, 2) and vr.dot_grid(513, False) == (2, 512, 2)
    assert vr.dot_grid(256, True) == (1, 256, 1) and vr.dot_grid(257, True) == (2, 512, 1)
    assert vr.dot_grid(262144, False) == (512, 131072, 2) and vr.dot_grid(262145, False) == (512, 131072, 3)
    assert vr.dot_grid(524289, False)[2] == 5 and vr.dot_grid(1000003, False)[2] == 8
    # complex: the grid is full from 131 072 elements on; the second load of a trip pair (h1) is live beyond a stride
    assert vr.dot_grid(130816, True) == (511, 130816, 1) and vr.dot_grid(130817, True) == (512, 131072, 1)
    assert vr.dot_grid(131072, True)[2] == 1 and vr.dot_grid(131073, True)[2] == 2
    assert vr.dot_grid(262144, True)[2] == 2 and vr.dot_grid(262145, True)[2] == 3
    assert vr.dot_grid(393216, True)[2] == 3 and vr.dot_grid(393217, True)[2] == 4
    assert vr.rms_grid(512) == (1, 256, 2) and vr.rms_grid(513) == (2, 512, 2)
    assert vr.rms_grid(262144) == (512, 131072, 2) and vr.rms_grid(262145)[2] == 3
    assert vr.ew_grid(1048576) == (4096, 1048576, 1) and vr.ew_grid(1048577)[2] == 2
    assert vr.ew_grid(2097157)[2] == 3 and vr.ew_grid(3145727)[2] == 3
    for lengths in (vr.REAL_RED_LENGTHS, vr.CPLX_RED_LENGTHS):
        assert max(lengths) == vr.RED_NMAX


@pytest.mark.parametrize("cplx", [False, True])
def test_emulated_order_is_exact_on_integer_vectors(cplx):
    x, y = vr.dot_vectors("int", cplx)
    for n in vr.red_lengths(cplx):
        if n > HOST_NMAX:
            continue
        want = np.vdot(x[:n], y[:n])            # integers: exact in any order
        (re, im), _ = vr.dot_reference("int", cplx, n)
        assert (re, im) == (want.real, want.imag), n
        assert vr.emulate_dot(x[:n], y[:n]) == (want.real, want.imag), n
        sq = np.vdot(x[:n], x[:n]).real
        assert vr.emulate_dot(x[:n], x[:n]) == (sq, 0.0), n


@pytest.mark.parametrize("cplx", [False, True])
def test_emulated_order_stays_within_the_dot_bound(cplx):
    x, y = vr.dot_vectors("f32", cplx)
    worst = 0.0
    for n in vr.red_lengths(cplx):
        if n > HOST_NMAX:
            continue
        got = vr.emulate_dot(x[:n], y[:n])
        ref, mags = vr.dot_reference("f32", cplx, n)
        for g, r, m in zip(got, ref, mags):
            bound = vr.dot_bound_factor(n, cplx) * m
            assert abs(g - r) <= bound, (n, g, r, bound)
            worst = max(worst, abs(g - r) / bound) if bound else worst
        sq, _ = vr.emulate_dot(x[:n], x[:n])
        (s_ref, _), _ = vr.dot_reference("f32", cplx, n, norm=True)
        assert abs(math.sqrt(sq) - math.sqrt(s_ref)) <= vr.nrm2_bound_factor(n, cplx) * math.sqrt(s_ref), n
    # the reference is not vacuous: naive float32 accumulation of the same data misses the bound by orders of magnitude
    n = 262145
    ref, mags = vr.dot_reference("f32", cplx, n)
    t = vr.dot_terms(x[:n], y[:n])[0]
    naive = float(np.sum([np.cumsum(a.astype(np.float32))[-1] for a in t]))
    assert abs(naive - ref[0]) > 100 * vr.dot_bound_factor(n, cplx) * mags[0]
    print(f"emulated dotc {'c128' if cplx else 'f64'}: worst observed/bound = {worst:.3f}")


@pytest.mark.parametrize("cplx", [False, True])
def test_emulated_order_on_the_cancelling_pair(cplx):
    x, y = vr.cancelling_pair(cplx)
    ref, mags = vr.exact_dot(x, y)
    n = len(x)
    assert n == vr.RED_NMAX
    for r, m in zip(ref, mags):
        if m:
            assert 1e-10 * m < abs(r) < 1e-8 * m            # heavy cancellation: exact dot ~ 1e-9 sum |x||y|
    got = vr.emulate_dot(x, y)
    for g, r, m in zip(got, ref, mags):
        assert abs(g - r) <= vr.dot_bound_factor(n, cplx) * m


@pytest.mark.parametrize("cplx", [False, True])
def test_emulated_scaled_rms_stays_within_its_bound(cplx):
    rng = np.random.default_rng(53 + cplx)
    worst = 0.0
    for n in vr.RMS_LENGTHS:
        for rtol, atol in vr.RMS_TOLS:
            x, y1, y2 = vr.rms_inputs(rng, n, cplx, away_from_zero=(atol == 0.0))
            ref = vr.rms_reference(x, y1, y2, rtol, atol)
            got = vr.emulate_scaled_rms(x, y1, y2, rtol, atol)
            rel = abs(float((np.longdouble(got) - ref) / ref))
            assert rel <= vr.rms_bound_factor(n), (n, rtol, atol, rel)
            worst = max(worst, rel / vr.rms_bound_factor(n))
    print(f"emulated scaled_rms {'c128' if cplx else 'f64'}: worst observed/bound = {worst:.3f}")


def test_scaled_rms_reference_survives_large_components():
    rng = np.random.default_rng(59)
    for n in (513, 262145):
        x, y1, y2 = vr.rms_overflow_inputs(rng, n)
        assert abs(float(vr.rms_reference(x, y1, y2, 1.0, 0.0)) - 1.0) <= vr.rms_bound_factor(n)
        assert abs(vr.emulate_scaled_rms(x, y1, y2, 1.0, 0.0) - 1.0) <= vr.rms_bound_factor(n)
        with np.errstate(over="ignore"):
            assert not np.isfinite(np.sqrt(x.real ** 2 + x.imag ** 2)).any()        # what hypot avoids
