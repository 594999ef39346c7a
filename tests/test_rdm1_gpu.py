"""``mpse_mps_rdm1`` on the GPU (``Engine.mps_rdm1``): chains of numpy arrays from a fixed seed against the same
contraction as ``numpy.einsum`` on the host, through the chain kernels and through the enqueued products.

Tolerance of an entry: 1e-12 * prod_i |A_i|_F^2.  Every environment obeys |E'|_F <= |A|_F^2 |E|_F, so that product
bounds every entry.  Rounding, as in tests/test_corr_gpu.py: per site an entry of a new environment sums p D products
twice in FP64 (unit roundoff 1.1e-16), the closing sum D^2 more: N (2 p D) u + D^2 u, at most 4 * 260 * 1.1e-16 + 4225 *
1.1e-16 = 5.8e-13 of the product for the shapes below (the limit cases; the others are far smaller).  float64 einsum
against clongdouble einsum differs by 1e-19 of the scale on these shapes, and the entries are 2e-4 of the scale on the
random chain, 2e-6 at bond 64: a wrong index, which changes an entry by its own size, lies 6 to 8 orders above the
tolerance.  Every case prints its largest ratio error / scale before it asserts."""
import ctypes as C

import numpy as np
import pytest

from chain_problems import _chain, _dev, took_path   # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu

BONDS, DS = (1, 3, 7, 10, 5, 2, 1), (2, 3, 2, 4, 2, 3)
ENV = "MPSE_RDM1_CHAIN"
PATHS = (("chain_kernel", "1"), ("enqueued", "0"))


def _host_rdms(sites):
    """([rho_i for every site], <psi|psi>, prod |A_i|_F^2) by einsum; the first index of L and R is the bra's"""
    a4 = [a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1]) for a in sites]
    n = len(a4)
    left = [np.ones((1, 1))]
    for a in a4[:-1]:
        left.append(np.einsum("bc,bsad,csae->de", left[-1], a.conj(), a, optimize=True))
    right = [np.ones((1, 1))]
    for a in a4[:0:-1]:
        right.append(np.einsum("bsad,csae,de->bc", a.conj(), a, right[-1], optimize=True))
    right = right[::-1]
    rho = [np.einsum("apgb,ac,cqgd,bd->pq", a4[i].conj(), left[i], a4[i], right[i], optimize=True) for i in range(n)]
    norm = np.einsum("bc,bsad,csad->", left[-1], a4[-1].conj(), a4[-1])
    return rho, complex(norm), float(np.prod([np.linalg.norm(a) ** 2 for a in sites]))


def _check(eng, dev, sel, path, ref, tol=None):
    """one call against numpy on the path the case means to take; returns the matrices.  tol: absolute, else 1e-12 of
    the scale"""
    rho, _, scale = ref
    got, s0, s1 = took_path(eng.mps_rdm1_stats, lambda: eng.mps_rdm1(dev, sel), path, len(dev))
    assert s1["matrices"] - s0["matrices"] == len(sel) and len(got) == len(sel)
    errs = [np.abs(g - rho[k]).max() for g, k in zip(got, sel)]
    what = f"/ scale = {max(errs) / scale:.2e}" if tol is None else f"= {max(errs):.2e} (absolute, <psi|psi> = 1)"
    print(f"{path} sel={list(sel) if len(sel) < 8 else len(sel)}: max |rdm1 - numpy| {what}")
    for g, k in zip(got, sel):
        assert g.shape == rho[k].shape and g.dtype == np.complex128
        assert np.all(np.abs(g - rho[k]) <= (1e-12 * scale if tol is None else tol)), (k, g, rho[k])
    return got


def _both_paths(eng, monkeypatch, sites, sel, ref, tol=None):
    dev = _dev(eng, sites)
    out = []
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        out.append(_check(eng, dev, sel, path, ref, tol))
    monkeypatch.delenv(ENV)
    return out


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


SELECTIONS = ((0, 2, 4), (0, 1, 2, 3, 4, 5), (3,), (0, 5), (1, 2))


@pytest.mark.parametrize("kind", ("real", "complex", "mixed"))
def test_selections_on_both_paths(eng, kind, monkeypatch):
    """bonds that are no power of two, d between 2 and 4; mixed: sites 2 and 3 complex.  Each selection through the chain
    kernels and through the enqueued products: both against numpy and against each other; Hermitian; one trace."""
    rng = np.random.default_rng(31)
    cplx = {"real": False, "complex": True, "mixed": [False, False, True, True, False, False]}[kind]
    sites = _chain(rng, BONDS, DS, cplx)
    ref = _host_rdms(sites)
    _, norm, scale = ref
    for sel in SELECTIONS:
        a, b = _both_paths(eng, monkeypatch, sites, sel, ref)
        for x, y in zip(a, b):
            assert np.all(np.abs(x - y) <= 2e-12 * scale)
            for m in (x, y):
                assert np.all(np.abs(m - m.conj().T) <= 2e-12 * scale)
                assert abs(np.trace(m) - norm) <= 2e-12 * scale          # trace(rho_i) = <psi|psi> for every i
                if kind == "real":
                    assert np.all(m.imag == 0)                           # exactly zero, not small


@pytest.mark.parametrize("cplx", (False, True))
def test_wave_assignment(eng, cplx, monkeypatch):
    """d = 17: one more than the 16 waves of a workgroup; d = 1: a site with one state; d = 5: an odd extent"""
    rng = np.random.default_rng(33)
    sites = _chain(rng, (1, 2, 3, 2, 1), (17, 1, 5, 2), cplx)
    _both_paths(eng, monkeypatch, sites, (0, 1, 2, 3), _host_rdms(sites))


@pytest.mark.parametrize("d, danc", ((2, 2), (2, 3)))
def test_density_operator_sites(eng, d, danc, monkeypatch):
    rng = np.random.default_rng(34)
    sites = _chain(rng, (1, 3, 4, 1), (d,) * 3, [True, False, True], danc=(danc,) * 3)
    ref = _host_rdms(sites)
    a, b = _both_paths(eng, monkeypatch, sites, (0, 1, 2), ref)
    for x, y in zip(a, b):
        assert np.all(np.abs(x - y) <= 2e-12 * ref[2])


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(eng, cplx, monkeypatch):
    """four sites of d = 2 with the inner bonds exactly at the limit of the path rule and one above, no switch set: the
    counters say which path ran.  Then the same at the limit of what fits the launches (every accumulator and all of
    the LDS plan in use) with MPSE_RDM1_CHAIN=1, which sends every chain that fits to the kernels."""
    from renormalizer_amd.engine import mps_rdm1_plan
    info = mps_rdm1_plan([[1, 2, 1, 1]], 1, cplx)[1]
    limit, fit = info["bond_limit"], info["bond_fit_limit"]
    rng = np.random.default_rng(35)
    monkeypatch.delenv(ENV, raising=False)
    cases = [(limit, "chain_kernel", None), (limit + 1, "enqueued", None), (fit, "chain_kernel", "1"),
             (fit + 1, "enqueued", "1")]
    for top, path, env in cases:
        if env is not None:
            monkeypatch.setenv(ENV, env)
        bonds = (1, top, top, top, 1)
        ok, info = mps_rdm1_plan([[bonds[i], 2, 1, bonds[i + 1]] for i in range(4)], 4, cplx)
        assert ok == (top <= limit) and (info["lds_bytes"] > 0) == ok and (info["lds_fit_bytes"] > 0) == (top <= fit)
        sites = [a / np.linalg.norm(a) for a in _chain(rng, bonds, (2,) * 4, cplx)]
        _check(eng, _dev(eng, sites), (0, 1, 2, 3), path, _host_rdms(sites))


def test_more_selected_sites_than_256(eng, monkeypatch):
    """300 sites, d = 2, bond 2, all selected: the grid of k_rdm1_sites has no cap.  Left-canonical isometries (QR of
    seeded complex Gaussians): <psi|psi> = 1, entries O(1).  Absolute tolerance 1e-12: the worst case is 300 * 8 * 1.1e-16
    * sqrt(2) = 3.7e-13; float64 against clongdouble einsum gave 1.9e-15."""
    rng = np.random.default_rng(36)
    n = 300
    bonds = (1,) + (2,) * (n - 1) + (1,)
    sites = []
    for i in range(n):
        g = rng.standard_normal((bonds[i] * 2, bonds[i + 1])) + 1j * rng.standard_normal((bonds[i] * 2, bonds[i + 1]))
        sites.append(np.linalg.qr(g)[0].reshape(bonds[i], 2, bonds[i + 1]))
    ref = _host_rdms(sites)
    assert abs(ref[1] - 1) < 1e-13
    for got in _both_paths(eng, monkeypatch, sites, tuple(range(n)), ref, tol=1e-12):
        assert all(abs(np.trace(m) - 1) <= 1e-12 for m in got)


def test_same_inputs_same_bits(eng, monkeypatch):
    rng = np.random.default_rng(37)
    dev = _dev(eng, _chain(rng, BONDS, DS, True))
    sel = (0, 1, 2, 3, 4, 5)
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        s0 = eng.mps_rdm1_stats()
        a, b = eng.mps_rdm1(dev, sel), eng.mps_rdm1(dev, sel)
        assert eng.mps_rdm1_stats()[path] - s0[path] == 2
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_refusals_leave_the_counters_alone(eng, monkeypatch):
    from renormalizer_amd.engine import MPSE_ERR_ARG, MPSE_ERR_SHAPE
    monkeypatch.delenv(ENV, raising=False)
    rng = np.random.default_rng(38)
    sites = _dev(eng, _chain(rng, (1, 3, 2, 1), (2, 2, 2), False))
    n = 3
    ptrs = (C.c_void_p * n)(*[t.ptr for t in sites])
    codes = (C.c_int * n)(*[t.code for t in sites])
    good = [1, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1]
    out = (C.c_double * 16)(*([7.0] * 16))

    def call(tab=good, sel=(0, 2), ptrs=ptrs, codes=codes, o=out, nsel=None):
        return eng.lib.mpse_mps_rdm1(eng.ctx, n, ptrs, codes, (C.c_int64 * 12)(*tab), len(sel) if nsel is None else nsel,
                                     (C.c_int * max(len(sel), 1))(*sel), o)

    s0, g0 = eng.mps_rdm1_stats(), eng.gemm_path_stats()
    bad_tables = ([1, 2, 1, 3, 4, 2, 1, 2, 2, 2, 1, 1],      # neighbours that do not match
                  [2, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1],      # first bond != 1
                  [1, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 2],      # last bond != 1
                  [1, 2, 0, 3, 3, 2, 1, 2, 2, 2, 1, 1],      # empty ancilla leg
                  [1, 0, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1])      # empty physical leg
    for tab in bad_tables:
        assert call(tab=tab) == MPSE_ERR_SHAPE, tab
    for sel in ((2, 0), (1, 1), (0, 3), (-1, 1)):                # descending, duplicated, out of range
        assert call(sel=sel) == MPSE_ERR_SHAPE, sel
    assert call(sel=(), nsel=0) == MPSE_ERR_ARG                   # an empty selection
    null_site = (C.c_void_p * n)(sites[0].ptr, None, sites[2].ptr)
    assert call(ptrs=null_site) == MPSE_ERR_ARG
    assert call(o=None) == MPSE_ERR_ARG
    assert call(codes=(C.c_int * n)(0, 7, 0)) == MPSE_ERR_ARG      # unknown dtype
    assert eng.mps_rdm1_stats() == s0 and eng.gemm_path_stats() == g0 and all(v == 7.0 for v in out)
    # the good call runs: two 2 x 2 matrices of a real chain, zero imaginary parts
    assert call() == 0 and all(out[i] != 7.0 for i in range(16)) and all(out[2 * i + 1] == 0.0 for i in range(8))
    s1 = eng.mps_rdm1_stats()
    assert s1["matrices"] - s0["matrices"] == 2 and s1["sites"] - s0["sites"] == 3
    for sel in ((2, 0), (1, 1), (0, 3), ()):
        with pytest.raises(ValueError):
            eng.mps_rdm1(sites, sel)
    assert eng.mps_rdm1_stats() == s1
