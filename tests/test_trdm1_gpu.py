"""``mpse_mps_trdm1`` on the GPU (``Engine.mps_trdm1``): two chains of numpy arrays from a fixed seed against the same
contraction as ``numpy.einsum`` on the host, through the chain kernels and through the enqueued products.

Tolerance of an entry: 1e-12 * prod_i |B_i|_F |K_i|_F.  Every environment obeys |E'|_F <= |B|_F |K|_F |E|_F, so that
product bounds every entry.  Rounding, as in tests/test_rdm1_gpu.py: per site an entry of a new environment sums p D
products twice in FP64 (unit roundoff 1.1e-16), the closing sum D^2 more: N (2 p D) u + D^2 u, at most 3 * 256 * 1.1e-16
+ 4096 * 1.1e-16 = 5.4e-13 of the product for the limit cases below (the others are far smaller).  A wrong index
changes an entry by its own size, orders above the tolerance.  Every case prints its largest ratio error / scale before
it asserts."""
import ctypes as C

import numpy as np
import pytest

from chain_problems import _chain, _dev, took_path   # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu

DS = (2, 3, 2, 4, 2, 3)
BONDS_A, BONDS_B = (1, 2, 5, 3, 4, 2, 1), (1, 3, 7, 10, 5, 2, 1)
DANC = (2, 1, 3, 1, 2, 1)
ENV = "MPSE_TRDM1_CHAIN"
PATHS = (("chain_kernel", "1"), ("enqueued", "0"))
SELECTIONS = ((0, 1, 2, 3, 4, 5), (0,), (5,), (1, 4))
KINDS = {"real": (False, False), "complex": (True, True),
         "mixed": ([False, False, True, True, False, False], [True, False, False, True, False, True]),
         "real bra": (False, True), "real ket": (True, False)}


def _host_trdms(bra, ket, conj):
    """([T_i for every site], <bra|ket>, prod |B_i|_F |K_i|_F) by einsum; the first index of L and R is the bra's"""
    b4 = [a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1]) for a in bra]
    b4 = [a.conj() for a in b4] if conj else b4
    k4 = [a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1]) for a in ket]
    n = len(b4)
    left = [np.ones((1, 1))]
    for b, k in zip(b4[:-1], k4[:-1]):
        left.append(np.einsum("bc,bsad,csae->de", left[-1], b, k, optimize=True))
    right = [np.ones((1, 1))]
    for b, k in zip(b4[:0:-1], k4[:0:-1]):
        right.append(np.einsum("bsad,csae,de->bc", b, k, right[-1], optimize=True))
    right = right[::-1]
    t = [np.einsum("apgb,ac,cqgd,bd->pq", b4[i], left[i], k4[i], right[i], optimize=True) for i in range(n)]
    ov = np.einsum("bc,bsad,csad->", left[-1], b4[-1], k4[-1])
    return t, complex(ov), float(np.prod([np.linalg.norm(a) for a in bra]) * np.prod([np.linalg.norm(a) for a in ket]))


def _check(eng, dbra, dket, sel, conj, path, ref):
    """one call against numpy on the path the case means to take; returns the matrices"""
    mats, _, scale = ref
    got, s0, s1 = took_path(eng.mps_trdm1_stats, lambda: eng.mps_trdm1(dbra, dket, sel, conj), path, len(dbra))
    assert s1["matrices"] - s0["matrices"] == len(sel) and len(got) == len(sel)
    errs = [np.abs(g - mats[k]).max() for g, k in zip(got, sel)]
    print(f"{path} conj={int(conj)} sel={list(sel)}: max |trdm1 - numpy| / scale = {max(errs) / scale:.2e}")
    for g, k in zip(got, sel):
        assert g.shape == mats[k].shape and g.dtype == np.complex128
        assert np.all(np.abs(g - mats[k]) <= 1e-12 * scale), (k, g, mats[k])
    return got


def _both_paths(eng, monkeypatch, bra, ket, sel, conj, ref):
    dbra, dket = _dev(eng, bra), _dev(eng, ket)
    out = []
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        out.append(_check(eng, dbra, dket, sel, conj, path, ref))
    monkeypatch.delenv(ENV)
    return out


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


@pytest.mark.parametrize("swapped", (False, True))
@pytest.mark.parametrize("kind", tuple(KINDS))
def test_selections_on_both_paths(eng, kind, swapped, monkeypatch):
    """bonds that are no power of two and differ between the chains at every inner bond (Db < Dk, swapped: Db > Dk), d
    between 2 and 4; mixed: complex sites 2, 3 of the bra and 0, 3, 5 of the ket.  Each selection with and without the
    conjugation through the chain kernels and through the enqueued products: both against numpy and against each other;
    one trace."""
    rng = np.random.default_rng(41)
    bb, kb = (BONDS_B, BONDS_A) if swapped else (BONDS_A, BONDS_B)
    bra, ket = _chain(rng, bb, DS, KINDS[kind][0]), _chain(rng, kb, DS, KINDS[kind][1])
    for conj in (0, 1):
        ref = _host_trdms(bra, ket, conj)
        _, ov, scale = ref
        for sel in SELECTIONS:
            a, b = _both_paths(eng, monkeypatch, bra, ket, sel, conj, ref)
            for x, y in zip(a, b):
                assert np.all(np.abs(x - y) <= 2e-12 * scale)
                for m in (x, y):
                    assert abs(np.trace(m) - ov) <= 2e-12 * scale         # trace(T_i) = <bra|ket> for every i
                    if kind == "real":
                        assert np.all(m.imag == 0)                          # exactly zero, not small


@pytest.mark.parametrize("swapped", (False, True))
def test_density_operator_sites(eng, swapped, monkeypatch):
    """ancilla legs of 2, 1, 3, 1, 2, 1 states, traced; mixed dtypes"""
    rng = np.random.default_rng(42)
    bb, kb = (BONDS_B, BONDS_A) if swapped else (BONDS_A, BONDS_B)
    bra, ket = _chain(rng, bb, DS, KINDS["mixed"][0], danc=DANC), _chain(rng, kb, DS, KINDS["mixed"][1], danc=DANC)
    for conj in (0, 1):
        ref = _host_trdms(bra, ket, conj)
        for sel in ((0, 1, 2, 3, 4, 5), (1, 4)):
            a, b = _both_paths(eng, monkeypatch, bra, ket, sel, conj, ref)
            for x, y in zip(a, b):
                assert np.all(np.abs(x - y) <= 2e-12 * ref[2])


@pytest.mark.parametrize("cplx", (False, True))
def test_wave_assignment(eng, cplx, monkeypatch):
    """d = 17: one more than the 16 waves of a workgroup; d = 1: a site with one state; d = 5: an odd extent"""
    rng = np.random.default_rng(43)
    ds = (17, 1, 5, 2)
    bra, ket = _chain(rng, (1, 2, 3, 2, 1), ds, cplx), _chain(rng, (1, 3, 2, 4, 1), ds, cplx)
    _both_paths(eng, monkeypatch, bra, ket, (0, 1, 2, 3), 1, _host_trdms(bra, ket, 1))


@pytest.mark.parametrize("db, dk", ((64, 64), (1, 64), (64, 1), (40, 40)))
def test_limit_cases(eng, db, dk, monkeypatch):
    """three complex sites of d = 2: every accumulator and nearly all of the LDS plan in use (64 on both chains), a
    product-state bra, a product-state ket (U of the middle site is 64 x 64 against environments of 64 elements), and
    bond 40 with 1600 entries, more than one accumulator per thread with the last ones idle"""
    from renormalizer_amd.engine import mps_trdm1_plan
    rng = np.random.default_rng(44)
    bb, kb = (1, db, db, 1), (1, dk, dk, 1)
    info = mps_trdm1_plan([[bb[i], kb[i], 2, 1, bb[i + 1], kb[i + 1]] for i in range(3)], 3, True)[1]
    assert info["lds_fit_bytes"] > 0
    bra = [a / np.linalg.norm(a) for a in _chain(rng, bb, (2,) * 3, True)]
    ket = [a / np.linalg.norm(a) for a in _chain(rng, kb, (2,) * 3, True)]
    _both_paths(eng, monkeypatch, bra, ket, (0, 1, 2), 1, _host_trdms(bra, ket, 1))


@pytest.mark.parametrize("cplx", (False, True))
def test_path_rule_without_the_switch(eng, cplx, monkeypatch):
    """four sites of d = 2 with the inner bonds of both chains at the limit of the path rule, then one above on the ket:
    the counters say which path ran"""
    from renormalizer_amd.engine import mps_trdm1_plan
    limit = mps_trdm1_plan([[1, 1, 2, 1, 1, 1]], 1, cplx)[1]["bond_limit"]
    rng = np.random.default_rng(45)
    monkeypatch.delenv(ENV, raising=False)
    for top, path in ((limit, "chain_kernel"), (limit + 1, "enqueued")):
        bb, kb = (1, limit, limit, limit, 1), (1, top, top, top, 1)
        ok = mps_trdm1_plan([[bb[i], kb[i], 2, 1, bb[i + 1], kb[i + 1]] for i in range(4)], 4, cplx)[0]
        assert ok == (path == "chain_kernel")
        bra = [a / np.linalg.norm(a) for a in _chain(rng, bb, (2,) * 4, cplx)]
        ket = [a / np.linalg.norm(a) for a in _chain(rng, kb, (2,) * 4, cplx)]
        _check(eng, _dev(eng, bra), _dev(eng, ket), (0, 1, 2, 3), 1, path, _host_trdms(bra, ket, 1))


def test_same_chain_is_rdm1_and_traces_are_the_overlap(eng, monkeypatch):
    rng = np.random.default_rng(46)
    ket = _chain(rng, BONDS_B, DS, True)
    bra = _chain(rng, BONDS_A, DS, [False, True, True, False, True, False])
    dket, dbra = _dev(eng, ket), _dev(eng, bra)
    sel = (0, 1, 2, 3, 4, 5)
    scale_kk = float(np.prod([np.linalg.norm(a) ** 2 for a in ket]))
    scale_bk = float(np.prod([np.linalg.norm(a) for a in bra]) * np.prod([np.linalg.norm(a) for a in ket]))
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        monkeypatch.setenv("MPSE_RDM1_CHAIN", env)
        rho = eng.mps_rdm1(dket, sel)
        t = eng.mps_trdm1(dket, dket, sel, True)
        err = max(np.abs(a - b).max() for a, b in zip(t, rho))
        print(f"{path}: max |trdm1(ket, ket) - rdm1(ket)| / scale = {err / scale_kk:.2e}")
        assert err <= 2e-12 * scale_kk
        for conj in (False, True):
            ov = eng.mps_overlap(dbra, dket, conj)
            tr = [np.trace(m) for m in eng.mps_trdm1(dbra, dket, sel, conj)]
            print(f"{path} conj={int(conj)}: max |trace - overlap| / scale = {max(abs(v - ov) for v in tr) / scale_bk:.2e}")
            assert all(abs(v - ov) <= 2e-12 * scale_bk for v in tr)


def test_same_inputs_same_bits(eng, monkeypatch):
    rng = np.random.default_rng(47)
    dbra, dket = _dev(eng, _chain(rng, BONDS_A, DS, True)), _dev(eng, _chain(rng, BONDS_B, DS, True))
    sel = (0, 1, 2, 3, 4, 5)
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        s0 = eng.mps_trdm1_stats()
        a, b = eng.mps_trdm1(dbra, dket, sel, True), eng.mps_trdm1(dbra, dket, sel, True)
        assert eng.mps_trdm1_stats()[path] - s0[path] == 2
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_refusals_leave_the_counters_alone(eng, monkeypatch):
    from renormalizer_amd.engine import MPSE_ERR_ARG, MPSE_ERR_SHAPE
    monkeypatch.delenv(ENV, raising=False)
    rng = np.random.default_rng(48)
    bra = _dev(eng, _chain(rng, (1, 3, 2, 1), (2, 2, 2), False))
    ket = _dev(eng, _chain(rng, (1, 2, 4, 1), (2, 2, 2), False))
    n = 3

    def arrs(sites):
        return (C.c_void_p * n)(*[t.ptr for t in sites]), (C.c_int * n)(*[t.code for t in sites])

    bp, bc = arrs(bra)
    kp, kc = arrs(ket)
    good = [1, 1, 2, 1, 3, 2, 3, 2, 2, 1, 2, 4, 2, 4, 2, 1, 1, 1]
    out = (C.c_double * 16)(*([7.0] * 16))

    def call(tab=good, sel=(0, 2), bp=bp, bc=bc, kp=kp, kc=kc, o=out, nsel=None):
        return eng.lib.mpse_mps_trdm1(eng.ctx, n, bp, bc, kp, kc, (C.c_int64 * 18)(*tab), 1,
                                      len(sel) if nsel is None else nsel, (C.c_int * max(len(sel), 1))(*sel), o)

    def changed(at, v):
        tab = list(good)
        tab[at] = v
        return tab

    s0, g0 = eng.mps_trdm1_stats(), eng.gemm_path_stats()
    # neighbours that do not match in the bra, in the ket; a first / last bond != 1 in either; empty legs
    for at, v in ((4, 4), (5, 3), (0, 2), (1, 2), (16, 2), (17, 2), (3, 0), (2, 0)):
        assert call(tab=changed(at, v)) == MPSE_ERR_SHAPE, (at, v)
    for sel in ((2, 0), (1, 1), (0, 3), (-1, 1)):                # descending, duplicated, out of range
        assert call(sel=sel) == MPSE_ERR_SHAPE, sel
    assert call(sel=(), nsel=0) == MPSE_ERR_ARG                   # an empty selection
    null_site = (C.c_void_p * n)(ket[0].ptr, None, ket[2].ptr)
    assert call(kp=null_site) == MPSE_ERR_ARG
    assert call(o=None) == MPSE_ERR_ARG
    assert call(bc=(C.c_int * n)(0, 7, 0)) == MPSE_ERR_ARG        # unknown dtype
    assert eng.mps_trdm1_stats() == s0 and eng.gemm_path_stats() == g0 and all(v == 7.0 for v in out)
    # the good call runs: two 2 x 2 matrices of two real chains, zero imaginary parts
    assert call() == 0 and all(out[i] != 7.0 for i in range(16)) and all(out[2 * i + 1] == 0.0 for i in range(8))
    s1 = eng.mps_trdm1_stats()
    assert s1["matrices"] - s0["matrices"] == 2 and s1["sites"] - s0["sites"] == 3
    for sel in ((2, 0), (1, 1), (0, 3), ()):
        with pytest.raises(ValueError):
            eng.mps_trdm1(bra, ket, sel, True)
    with pytest.raises(ValueError):
        eng.mps_trdm1(bra, ket[:2], (0,), True)
    assert eng.mps_trdm1_stats() == s1
