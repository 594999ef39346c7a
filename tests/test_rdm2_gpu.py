"""``mpse_mps_rdm2`` on the GPU (``Engine.mps_rdm2``): chains of numpy arrays from a fixed seed against the plain
contraction as ``numpy.einsum`` on the host - walk E to site k, open with |p><p'|, transfer, close with |q><q'| against
the right environment - through the chain kernels, through the enqueued products and through the enqueued products in
chunks of single rows.

Tolerance of an entry: 1e-12 * prod_i |A_i|_F^2, the bound derived in the docstring of tests/test_corr_gpu.py for these
very extents; the elementary matrices |p><p'| and |q><q'| that take the place of X_k and Y_l there have norm 1.  The
paths must agree among each other to twice that.  Every case prints its largest error / scale before it asserts."""
import ctypes as C

import numpy as np
import pytest

from chain_problems import _chain, _dev, took_path   # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu

BONDS, DS = (1, 3, 7, 10, 5, 2, 1), (2, 3, 2, 4, 2, 3)
CHAIN, STACK = "MPSE_RDM2_CHAIN", "MPSE_RDM2_STACK_BYTES"
# (name, counter of the path, MPSE_RDM2_CHAIN, MPSE_RDM2_STACK_BYTES): with a bound of one byte every chunk of the
# enqueued path holds one row, a part of one opening site (every d here is at least 2)
PATHS = (("kernels", "chain_kernel", "1", None), ("enqueued", "enqueued", "0", None), ("rows", "enqueued", "0", "1"))
SELECTIONS = ((0, 2, 4), (0, 1, 2, 3, 4, 5), (0, 5), (1, 2))


def _host_rdm2(sites, conj_bra=True):
    """({(k, l): rho[p, p', q, q'] for all pairs of sites}, <psi|psi>, prod |A_i|_F^2) by einsum; the first index of
    every environment is the bra's"""
    a4 = [a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1]) for a in sites]
    bra = [a.conj() if conj_bra else a for a in a4]
    n = len(a4)
    left = [np.ones((1, 1))]
    for b, a in zip(bra[:-1], a4[:-1]):
        left.append(np.einsum("bc,bsad,csae->de", left[-1], b, a, optimize=True))
    right = [np.ones((1, 1))]
    for b, a in zip(bra[:0:-1], a4[:0:-1]):
        right.append(np.einsum("bsad,csae,de->bc", b, a, right[-1], optimize=True))
    right = right[::-1]            # right[i]: the environment right of site i
    rho = {}
    for k in range(n - 1):
        t = np.einsum("bc,bpgd,cqge->pqde", left[k], bra[k], a4[k], optimize=True)
        for l in range(k + 1, n):
            rho[(k, l)] = np.einsum("pqbc,bsgd,ctge,de->pqst", t, bra[l], a4[l], right[l], optimize=True)
            t = np.einsum("pqbc,bsgd,csge->pqde", t, bra[l], a4[l], optimize=True)
    norm = np.einsum("bc,bsad,csad->", left[-1], bra[-1], a4[-1])
    return rho, complex(norm), float(np.prod([np.linalg.norm(a) ** 2 for a in sites]))


def _set_path(monkeypatch, chain, stack):
    for name, value in ((CHAIN, chain), (STACK, stack)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _check(eng, dev, sel, name, counter, ref):
    """one call against numpy on the path the case means to take; returns the blocks"""
    rho, _, scale = ref
    got, s0, s1 = took_path(eng.mps_rdm2_stats, lambda: eng.mps_rdm2(dev, sel), counter, len(dev))
    pairs = [(k, l) for i, k in enumerate(sel) for l in sel[i + 1:]]
    assert s1["pairs"] - s0["pairs"] == len(pairs) and list(got) == pairs
    err = max(np.abs(got[kl] - rho[kl]).max() for kl in pairs)
    print(f"{name} sel={list(sel)}: max |rdm2 - numpy| / scale = {err / scale:.2e}")
    for kl in pairs:
        assert got[kl].shape == rho[kl].shape and got[kl].dtype == np.complex128
        assert np.all(np.abs(got[kl] - rho[kl]) <= 1e-12 * scale), (kl, got[kl], rho[kl])
    return got


def _all_paths(eng, monkeypatch, sites, sel, ref, paths=PATHS):
    dev = _dev(eng, sites)
    out = []
    for name, counter, chain, stack in paths:
        _set_path(monkeypatch, chain, stack)
        out.append(_check(eng, dev, sel, name, counter, ref))
    _set_path(monkeypatch, None, None)
    scale = ref[2]
    for other in out[1:]:
        for kl, m in out[0].items():
            assert np.all(np.abs(m - other[kl]) <= 2e-12 * scale), kl
    return out


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


@pytest.mark.parametrize("kind", ("real", "complex", "mixed"))
def test_selections_on_every_path(eng, kind, monkeypatch):
    """bonds that are no power of two, d between 2 and 4 with d_k != d_l for most pairs; mixed: sites 2 and 3 complex.
    Each selection through the kernels, the enqueued products and the enqueued products one row per chunk: against
    numpy and against each other; every matrix [(p, q), (p', q')] Hermitian with the chain's norm square as trace"""
    rng = np.random.default_rng(21)
    cplx = {"real": False, "complex": True, "mixed": [False, False, True, True, False, False]}[kind]
    sites = _chain(rng, BONDS, DS, cplx)
    ref = _host_rdm2(sites)
    _, norm, scale = ref
    for sel in SELECTIONS:
        for got in _all_paths(eng, monkeypatch, sites, sel, ref):
            for (k, l), r in got.items():
                m = r.transpose(0, 2, 1, 3).reshape(DS[k] * DS[l], DS[k] * DS[l])
                assert np.all(np.abs(m - m.conj().T) <= 1e-12 * scale)
                assert abs(np.trace(m) - norm) <= 1e-12 * scale
                if kind == "real":
                    assert np.all(r.imag == 0)                           # exactly zero, not small


def test_slots_are_not_interchangeable():
    """the references with p / p' swapped, with q / q' swapped, with the bra unconjugated and (where d_k = d_l) with the
    pair block transposed lie far outside the tolerance of the right one, for every pair: the checks above can tell them
    apart.  (Smallest difference on the CPU for this seed: 2.9e-5 of the scale.)"""
    rng = np.random.default_rng(21)
    sites = _chain(rng, BONDS, DS, True)
    rho, _, scale = _host_rdm2(sites)
    plain = _host_rdm2(sites, conj_bra=False)[0]
    smallest = np.inf
    for (k, l), r in rho.items():
        others = [r.transpose(1, 0, 2, 3), r.transpose(0, 1, 3, 2), plain[(k, l)]]
        if DS[k] == DS[l]:
            others.append(r.transpose(2, 3, 0, 1))
        smallest = min([smallest] + [np.abs(o - r).max() for o in others])
    print(f"smallest |wrong reference - reference| / scale = {smallest / scale:.2e}")
    assert smallest > 1e-6 * scale


@pytest.mark.parametrize("d, danc", ((2, 2), (2, 3)))
def test_density_operator_sites(eng, d, danc, monkeypatch):
    rng = np.random.default_rng(23)
    sites = _chain(rng, (1, 3, 4, 1), (d,) * 3, [True, False, True], danc=(danc,) * 3)
    _all_paths(eng, monkeypatch, sites, (0, 1, 2), _host_rdm2(sites), PATHS[:2])


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(eng, cplx, monkeypatch):
    """four sites of d = 2 with the inner bonds exactly at the limit of the path rule and one above, no switch set: the
    counters say which path ran.  Then the same at the limit of what fits the launches (every accumulator and all of
    the LDS plan in use) with MPSE_RDM2_CHAIN=1, which sends every chain that fits to the kernels."""
    from renormalizer_amd.engine import mps_rdm2_plan
    sel = (0, 1, 2, 3)
    info = mps_rdm2_plan([[1, 2, 1, 1]] * 2, (0, 1), cplx)[1]
    limit, fit = info["bond_limit"], info["bond_fit_limit"]
    rng = np.random.default_rng(24)
    cases = [(limit, "chain_kernel", None), (limit + 1, "enqueued", None), (fit, "chain_kernel", "1"),
             (fit + 1, "enqueued", "1")]
    for top, counter, env in cases:
        _set_path(monkeypatch, env, None)
        bonds = (1, top, top, top, 1)
        ok, info = mps_rdm2_plan([[bonds[i], 2, 1, bonds[i + 1]] for i in range(4)], sel, cplx)
        assert ok == (top <= limit) and (info["lds_bytes"] > 0) == ok and (info["lds_fit_bytes"] > 0) == (top <= fit)
        sites = [a / np.linalg.norm(a) for a in _chain(rng, bonds, (2,) * 4, cplx)]
        _check(eng, _dev(eng, sites), sel, f"bond {top}", counter, _host_rdm2(sites))


def test_same_inputs_same_bits(eng, monkeypatch):
    rng = np.random.default_rng(25)
    dev = _dev(eng, _chain(rng, BONDS, DS, True))
    sel = (0, 1, 2, 3, 4, 5)
    for _, counter, chain, stack in PATHS:
        _set_path(monkeypatch, chain, stack)
        s0 = eng.mps_rdm2_stats()
        a, b = eng.mps_rdm2(dev, sel), eng.mps_rdm2(dev, sel)
        assert eng.mps_rdm2_stats()[counter] - s0[counter] == 2
        assert all(a[kl].tobytes() == b[kl].tobytes() for kl in a)


def test_refusals_leave_the_counters_alone(eng, monkeypatch):
    """the table of bad dims and selections of tests/test_corr_gpu.py, and a selection of one site"""
    from renormalizer_amd.engine import MPSE_ERR_ARG, MPSE_ERR_SHAPE
    _set_path(monkeypatch, None, None)
    rng = np.random.default_rng(26)
    sites = _dev(eng, _chain(rng, (1, 3, 2, 1), (2, 2, 2), False))
    n = 3
    ptrs = (C.c_void_p * n)(*[t.ptr for t in sites])
    codes = (C.c_int * n)(*[t.code for t in sites])
    good = [1, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1]
    out = (C.c_double * 32)(*([7.0] * 32))

    def call(tab=good, sel=(0, 2), ptrs=ptrs, codes=codes, o=out, nsel=None):
        return eng.lib.mpse_mps_rdm2(eng.ctx, n, ptrs, codes, (C.c_int64 * 12)(*tab), len(sel) if nsel is None else nsel,
                                     (C.c_int * max(len(sel), 1))(*sel), o)

    s0, g0 = eng.mps_rdm2_stats(), eng.gemm_path_stats()
    bad_tables = ([1, 2, 1, 3, 4, 2, 1, 2, 2, 2, 1, 1],      # neighbours that do not match
                  [2, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1],      # first bond != 1
                  [1, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 2],      # last bond != 1
                  [1, 2, 0, 3, 3, 2, 1, 2, 2, 2, 1, 1],      # empty ancilla leg
                  [1, 0, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1])      # empty physical leg
    for tab in bad_tables:
        assert call(tab=tab) == MPSE_ERR_SHAPE, tab
    for sel in ((2, 0), (1, 1), (0, 3), (-1, 1)):                # descending, duplicated, out of range
        assert call(sel=sel) == MPSE_ERR_SHAPE, sel
    assert call(sel=(1,)) == MPSE_ERR_ARG                         # one site is no pair
    assert call(sel=(), nsel=0) == MPSE_ERR_ARG
    null_site = (C.c_void_p * n)(sites[0].ptr, None, sites[2].ptr)
    assert call(ptrs=null_site) == MPSE_ERR_ARG
    assert call(o=None) == MPSE_ERR_ARG
    assert call(codes=(C.c_int * n)(0, 7, 0)) == MPSE_ERR_ARG      # unknown dtype
    assert eng.mps_rdm2_stats() == s0 and eng.gemm_path_stats() == g0 and all(v == 7.0 for v in out)
    # the good call runs: one 2 x 2 x 2 x 2 block of a real chain, zero imaginary parts
    assert call() == 0 and all(out[2 * i] != 7.0 for i in range(16)) and all(out[2 * i + 1] == 0.0 for i in range(16))
    s1 = eng.mps_rdm2_stats()
    assert s1["pairs"] - s0["pairs"] == 1 and s1["sites"] - s0["sites"] == 3
    for sel in ((2, 0), (1, 1), (0, 3), (), (1,)):
        with pytest.raises(ValueError):
            eng.mps_rdm2(sites, sel)
    assert eng.mps_rdm2_stats() == s1
