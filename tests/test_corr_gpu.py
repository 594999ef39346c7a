"""``mpse_mps_corr`` on the GPU (``Engine.mps_corr``): chains of numpy arrays from a fixed seed, random non-Hermitian
complex local matrices X (open), Y (close), Z (diagonal), against the same contraction as ``numpy.einsum`` on the host.

Tolerance of an entry: 1e-12 * prod_i |A_i|_F^2 * |X_k|_F |Y_l|_F (the diagonal: |Z_k|_F for the two).  Every
environment obeys |E'|_F <= |A|_F^2 |O|_F |E|_F, so that product bounds the entry.  Per site an entry of the new
environment sums p D <= 2 * 65 (limit cases) resp. 4 * 10 products twice, in FP64 (unit roundoff 1.1e-16), the closing
sums D^2 <= 4225 more: N (2 p D) u + D^2 u <= 4 * 260 * 1.1e-16 + 4225 * 1.1e-16 = 5.8e-13 of the product at the very
worst, rounding errors all of one sign.  Every case prints its largest ratio error / scale before it asserts."""
import ctypes as C

import numpy as np
import pytest

from chain_problems import _chain, _dev, took_path   # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu

BONDS, DS = (1, 3, 7, 10, 5, 2, 1), (2, 3, 2, 4, 2, 3)


def _mats(rng, sites, sel, cplx=True):
    out = []
    for _ in range(3):
        ms = []
        for k in sel:
            d = sites[k].shape[1]
            m = rng.standard_normal((d, d))
            ms.append(m + 1j * rng.standard_normal((d, d)) if cplx else m)
        out.append(ms)
    return out


def _host_entry(sites, ops):
    e = np.ones((1, 1))
    for i, a in enumerate(sites):
        a4 = a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1])
        o = ops.get(i, np.eye(a.shape[1]))
        e = np.einsum("bc,bsad,st,ctae->de", e, a4.conj(), o, a4, optimize=True)
    return complex(e[0, 0])


def _host_corr(sites, sel, X, Y, Z):
    """(values, scales), the lower triangle zero"""
    n = len(sel)
    ref, scale = np.zeros((n, n), complex), np.zeros((n, n))
    base = float(np.prod([np.linalg.norm(a) ** 2 for a in sites]))
    for k in range(n):
        ref[k, k] = _host_entry(sites, {sel[k]: Z[k]})
        scale[k, k] = base * np.linalg.norm(Z[k])
        for l in range(k + 1, n):
            ref[k, l] = _host_entry(sites, {sel[k]: X[k], sel[l]: Y[l]})
            scale[k, l] = base * np.linalg.norm(X[k]) * np.linalg.norm(Y[l])
    return ref, scale


def _check(eng, sites, sel, mats, path, ref=None):
    """one call against numpy on the path the case means to take; returns (values, reference, scales)"""
    X, Y, Z = mats
    if ref is None:
        ref = _host_corr(sites, sel, X, Y, Z)
    val, scale = ref
    dev = _dev(eng, sites)
    got, s0, s1 = took_path(eng.mps_corr_stats, lambda: eng.mps_corr(dev, sel, X, Y, Z), path, len(sites))
    n = len(sel)
    iu = np.triu_indices(n)
    ratio = (np.abs(got - val)[iu] / scale[iu]).max()
    print(f"{path} sel={list(sel)}: max |corr - numpy| / scale = {ratio:.2e}")
    assert s1["entries"] - s0["entries"] == n * (n + 1) // 2
    assert np.all(np.abs(got - val)[iu] <= 1e-12 * scale[iu]), (got, val)
    assert np.all(got[np.tril_indices(n, -1)] == 0)          # exactly zero, not small
    return got, ref


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


SELECTIONS = ((0, 2, 4), (0, 1, 2, 3, 4, 5), (3,), (0, 5), (1, 2))


@pytest.mark.parametrize("kind", ("real", "complex", "mixed", "real_ops"))
def test_selections_on_both_paths(eng, kind, monkeypatch):
    """bonds that are no power of two, d between 2 and 4; mixed: sites 2 and 3 complex; real_ops: real sites and real
    local matrices, the real instantiation of the kernels.  Each selection through the chain kernels, then through the
    enqueued products (MPSE_CORR_CHAIN=0): both against numpy and against each other."""
    rng = np.random.default_rng(21)
    cplx = {"real": False, "complex": True, "mixed": [False, False, True, True, False, False], "real_ops": False}[kind]
    sites = _chain(rng, BONDS, DS, cplx)
    for sel in SELECTIONS:
        mats = _mats(rng, sites, sel, cplx=kind != "real_ops")
        a, ref = _check(eng, sites, sel, mats, "chain_kernel")
        monkeypatch.setenv("MPSE_CORR_CHAIN", "0")
        b, _ = _check(eng, sites, sel, mats, "enqueued", ref)
        monkeypatch.delenv("MPSE_CORR_CHAIN")
        assert np.all(np.abs(a - b) <= 2e-12 * ref[1])
        if kind == "real_ops":
            assert np.all(a.imag == 0) and np.all(b.imag == 0)


def test_slots_are_not_interchangeable(eng):
    """the reference values of X/Y swapped, of the transposed matrices and of the unconjugated bra lie far outside the
    tolerance of the ones asked for: the checks above can tell them apart"""
    rng = np.random.default_rng(22)
    sites = _chain(rng, BONDS, DS, True)
    sel = (0, 2, 4)
    X, Y, Z = _mats(rng, sites, sel)
    val, scale = _host_corr(sites, sel, X, Y, Z)
    for other in (_host_corr(sites, sel, Y, X, Z), _host_corr(sites, sel, [m.T for m in X], [m.T for m in Y], Z),
                  _host_corr(sites, sel, X, Y, X)):
        assert np.abs(other[0] - val).max() > 1e-6 * scale.max()


@pytest.mark.parametrize("d, danc", ((2, 2), (2, 3)))
def test_density_operator_sites(eng, d, danc, monkeypatch):
    rng = np.random.default_rng(23)
    sites = _chain(rng, (1, 3, 4, 1), (d,) * 3, [True, False, True], danc=(danc,) * 3)
    sel = (0, 1, 2)
    mats = _mats(rng, sites, sel)
    a, ref = _check(eng, sites, sel, mats, "chain_kernel")
    monkeypatch.setenv("MPSE_CORR_CHAIN", "0")
    b, _ = _check(eng, sites, sel, mats, "enqueued", ref)
    assert np.all(np.abs(a - b) <= 2e-12 * ref[1])


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(eng, cplx, monkeypatch):
    """four sites of d = 2 with the inner bonds exactly at the limit of the path rule and one above: the counters say
    which path ran.  Then the same at the limit of what fits the launches (every accumulator and all of the LDS plan in
    use) with MPSE_CORR_CHAIN=1, which sends every chain that fits to the kernels."""
    from renormalizer_amd.engine import mps_corr_plan
    info = mps_corr_plan([[1, 2, 1, 1]], 1, cplx)[1]
    limit, fit = info["bond_limit"], info["bond_fit_limit"]
    rng = np.random.default_rng(24)
    cases = [(limit, "chain_kernel", None), (limit + 1, "enqueued", None), (fit, "chain_kernel", "1"),
             (fit + 1, "enqueued", "1")]
    for top, path, env in cases:
        if env is not None:
            monkeypatch.setenv("MPSE_CORR_CHAIN", env)
        bonds = (1, top, top, top, 1)
        ok, info = mps_corr_plan([[bonds[i], 2, 1, bonds[i + 1]] for i in range(4)], 3, True)
        assert ok == (top <= limit) and (info["lds_bytes"] > 0) == ok and (info["lds_fit_bytes"] > 0) == (top <= fit)
        sites = [a / np.linalg.norm(a) for a in _chain(rng, bonds, (2,) * 4, cplx)]
        sel = (0, 1, 3)
        _check(eng, sites, sel, _mats(rng, sites, sel), path)


def test_same_inputs_same_bits(eng, monkeypatch):
    rng = np.random.default_rng(25)
    sites = _chain(rng, BONDS, DS, True)
    dev = _dev(eng, sites)
    sel = (0, 1, 2, 3, 4, 5)
    X, Y, Z = _mats(rng, sites, sel)
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("MPSE_CORR_CHAIN", env)
        a, b = eng.mps_corr(dev, sel, X, Y, Z), eng.mps_corr(dev, sel, X, Y, Z)
        assert a.tobytes() == b.tobytes()
    assert eng.mps_corr_stats()["enqueued"] >= 2


def test_refusals_leave_the_counters_alone(eng):
    from renormalizer_amd.engine import MPSE_ERR_ARG, MPSE_ERR_SHAPE
    rng = np.random.default_rng(26)
    sites = _dev(eng, _chain(rng, (1, 3, 2, 1), (2, 2, 2), False))
    n = 3
    ptrs = (C.c_void_p * n)(*[t.ptr for t in sites])
    codes = (C.c_int * n)(*[t.code for t in sites])
    good = [1, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1]
    mat = (C.c_double * (2 * 4 * 3))(*([0.5] * 24))
    out = (C.c_double * 18)(*([7.0] * 18))

    def call(tab=good, sel=(0, 2), ptrs=ptrs, codes=codes, x=mat, o=out):
        return eng.lib.mpse_mps_corr(eng.ctx, n, ptrs, codes, (C.c_int64 * 12)(*tab), len(sel), (C.c_int * max(len(sel), 1))(*sel),
                                     x, mat, mat, o)

    s0, g0 = eng.mps_corr_stats(), eng.gemm_path_stats()
    bad_tables = ([1, 2, 1, 3, 4, 2, 1, 2, 2, 2, 1, 1],      # neighbours that do not match
                  [2, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1],      # first bond != 1
                  [1, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 2],      # last bond != 1
                  [1, 2, 0, 3, 3, 2, 1, 2, 2, 2, 1, 1],      # empty ancilla leg
                  [1, 0, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1])      # empty physical leg
    for tab in bad_tables:
        assert call(tab=tab) == MPSE_ERR_SHAPE, tab
    for sel in ((2, 0), (1, 1), (0, 3), (-1, 1)):                # descending, duplicated, out of range
        assert call(sel=sel) == MPSE_ERR_SHAPE, sel
    null_site = (C.c_void_p * n)(sites[0].ptr, None, sites[2].ptr)
    assert call(ptrs=null_site) == MPSE_ERR_ARG
    assert call(x=None) == MPSE_ERR_ARG and call(o=None) == MPSE_ERR_ARG
    assert call(codes=(C.c_int * n)(0, 7, 0)) == MPSE_ERR_ARG      # unknown dtype
    assert eng.mps_corr_stats() == s0 and eng.gemm_path_stats() == g0 and all(v == 7.0 for v in out)
    assert call() == 0 and out[4] == 0.0 and out[5] == 0.0 and out[0] != 7.0    # the good call runs; entry [1, 0] is zero
    with pytest.raises(ValueError):
        eng.mps_corr(sites, (0, 2), [np.eye(3)] * 2, [np.eye(2)] * 2, [np.eye(2)] * 2)
