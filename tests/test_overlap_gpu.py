"""``mpse_mps_overlap`` on the GPU (``Engine.mps_overlap`` / ``Mps.overlap``): chains of numpy arrays from a fixed seed
against the same contraction in numpy on the host and against ``Mps.dot``.

Tolerance: 1e-12 * prod_i |B_i|_F |K_i|_F.  Every path sums at most p * D <= 8 * 65 products per entry and site in
FP64 (unit roundoff 1.1e-16) and |E_{i+1}|_F <= |B_i|_F |E_i|_F |K_i|_F, so the error of a chain of N <= 5 sites is of
the order N * 520 * 1.1e-16 = 3e-13 of that product at the very worst.  Every case prints its ratio
error / (prod |B| |K|) before it asserts; the bound has not been confirmed on a GPU run yet."""
import ctypes as C

import numpy as np
import pytest

from chain_problems import _chain, _dev, took_path   # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu


def _host_overlap(bra, ket, conj_bra):
    e = np.ones((1, 1))
    for b, k in zip(bra, ket):
        b3, k3 = b.reshape(b.shape[0], -1, b.shape[-1]), k.reshape(k.shape[0], -1, k.shape[-1])
        if conj_bra:
            b3 = b3.conj()
        e = np.einsum("bsc,bk,ksl->cl", b3, e, k3, optimize=True)
    return complex(e[0, 0])


def _scale(bra, ket):
    return float(np.prod([np.linalg.norm(b) * np.linalg.norm(k) for b, k in zip(bra, ket)]))


def _as_mps(eng, arrays):
    from renormalizer_amd.mps.mps import Mps
    m = Mps()
    m._mp = _dev(eng, arrays)
    m.dtype = np.dtype(np.complex128 if any(np.iscomplexobj(a) for a in arrays) else np.float64)
    return m


def _check(eng, bra, ket, conj_bra, path):
    """overlap against numpy and against Mps.dot, on the path the case means to take; returns the value"""
    mb, mk = _as_mps(eng, bra), _as_mps(eng, ket)
    ref = _host_overlap(bra, ket, conj_bra)
    tol = 1e-12 * _scale(bra, ket)
    got, _, _ = took_path(eng.mps_overlap_stats, lambda: mb.overlap(mk, self_is_conj=not conj_bra), path, len(bra))
    dot = mb.dot(mk, self_is_conj=not conj_bra)
    print(f"{path}: |overlap - numpy| / scale = {abs(got - ref) / _scale(bra, ket):.2e}, "
          f"|overlap - dot| / scale = {abs(got - dot) / _scale(bra, ket):.2e}")
    assert abs(got - ref) <= tol, (got, ref, tol)
    assert abs(got - dot) <= tol, (got, dot, tol)
    return got


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


BRA5, KET5, P5 = (1, 2, 5, 3, 2, 1), (1, 3, 4, 4, 3, 1), (2, 3, 2, 3, 2)


def test_single_site_and_pair(eng):
    rng = np.random.default_rng(11)
    _check(eng, _chain(rng, (1, 1), (3,), False), _chain(rng, (1, 1), (3,), False), False, "chain_kernel")
    _check(eng, _chain(rng, (1, 1), (3,), True), _chain(rng, (1, 1), (3,), True), True, "chain_kernel")
    _check(eng, _chain(rng, (1, 4, 1), (2, 3), False), _chain(rng, (1, 3, 1), (2, 3), True), False, "chain_kernel")


@pytest.mark.parametrize("kind", ("real", "complex", "mixed"))
def test_rectangular_chain(eng, kind):
    """bra bonds != ket bonds, no power of two, p alternating 2 / 3; mixed: a real bra and a ket that turns complex at
    site 2 and real again at site 4"""
    rng = np.random.default_rng(12)
    bra_c = {"real": False, "complex": True, "mixed": False}[kind]
    ket_c = {"real": False, "complex": True, "mixed": [False, False, True, True, False]}[kind]
    bra, ket = _chain(rng, BRA5, P5, bra_c), _chain(rng, KET5, P5, ket_c)
    for conj_bra in (False, True):
        _check(eng, bra, ket, conj_bra, "chain_kernel")


def test_conjugation_differs_on_complex_data(eng):
    rng = np.random.default_rng(13)
    bra, ket = _chain(rng, BRA5, P5, True), _chain(rng, KET5, P5, True)
    plain = _check(eng, bra, ket, False, "chain_kernel")
    conj = _check(eng, bra, ket, True, "chain_kernel")
    # each is within the tolerance of its own numpy value; the two numpy values are further apart than that
    assert abs(_host_overlap(bra, ket, False) - _host_overlap(bra, ket, True)) > 1e-6 * abs(plain)
    assert abs(plain - conj) > 2e-12 * _scale(bra, ket)
    # a complex bra in a mixed chain is conjugated site by site as well
    bra_m = _chain(rng, BRA5, P5, [True, False, True, False, False])
    assert abs(_check(eng, bra_m, ket, False, "chain_kernel") - _check(eng, bra_m, ket, True, "chain_kernel")) > 0


@pytest.mark.parametrize("d", (2, 3))
def test_mpdm_shaped_sites(eng, d):
    rng = np.random.default_rng(14)
    bra = _chain(rng, (1, 3, 5, 1), ((d, d),) * 3, True)
    ket = _chain(rng, (1, 4, 2, 1), ((d, d),) * 3, False)
    _check(eng, bra, ket, True, "chain_kernel")


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(eng, cplx):
    """one bond exactly at the chain-kernel limit (every accumulator and all of E in use) and its twin one above"""
    from renormalizer_amd.engine import mps_overlap_plan
    limit = mps_overlap_plan([[1, 1, 2, 1, 1]], cplx)[1]["bond_limit"]
    rng = np.random.default_rng(15)
    vals = []
    for top, path in ((limit, "chain_kernel"), (limit + 1, "enqueued")):
        bonds_b, bonds_k = (1, 7, top, 5, 1), (1, 6, top, limit, 1)
        ok, info = mps_overlap_plan([[bonds_b[i], bonds_k[i], 2, bonds_b[i + 1], bonds_k[i + 1]] for i in range(4)], cplx)
        assert ok == (path == "chain_kernel") and (info["lds_bytes"] > 0) == ok
        bra, ket = _chain(rng, bonds_b, (2,) * 4, cplx), _chain(rng, bonds_k, (2,) * 4, cplx)
        # scaled so that the product of the norms stays of order one
        bra = [a / np.linalg.norm(a) for a in bra]
        ket = [a / np.linalg.norm(a) for a in ket]
        vals.append((_check(eng, bra, ket, True, path), bra, ket))
    # the twin, cut back to the limit, through both paths: same chain, two summation orders
    _, bra, ket = vals[1]
    bra_cut = [bra[0], bra[1][:, :, :limit].copy(), bra[2][:limit].copy(), bra[3]]
    ket_cut = [ket[0], ket[1][:, :, :limit].copy(), ket[2][:limit].copy(), ket[3]]
    a = _check(eng, bra_cut, ket_cut, True, "chain_kernel")
    assert abs(a - _host_overlap(bra_cut, ket_cut, True)) <= 1e-12 * _scale(bra_cut, ket_cut)


def test_norm_of_a_canonical_random_mps(eng):
    from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity
    from renormalizer_amd.mps.mps import Mps
    ph = Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.27), 4)
    model = HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(3.0e-2), 3)
    mps = Mps.random(model, 1, 8, rng=np.random.default_rng(16))
    mps.canonicalise()
    mps.normalize("mps_only")
    s0 = eng.mps_overlap_stats()
    val = mps.overlap(mps, self_is_conj=False)
    assert eng.mps_overlap_stats()["chain_kernel"] == s0["chain_kernel"] + 1
    assert abs(val - 1.0) < 1e-12, val


def test_same_inputs_same_bits(eng):
    rng = np.random.default_rng(17)
    for bonds_b, bonds_k in ((BRA5, KET5), ((1, 9, 70, 9, 2, 1), (1, 3, 66, 4, 3, 1))):
        mb, mk = _as_mps(eng, _chain(rng, bonds_b, P5, True)), _as_mps(eng, _chain(rng, bonds_k, P5, True))
        a, b = mb.overlap(mk, self_is_conj=False), mb.overlap(mk, self_is_conj=False)
        assert a.real.hex() == b.real.hex() and a.imag.hex() == b.imag.hex()


def test_inconsistent_dims_are_refused_without_device_work(eng):
    from renormalizer_amd.engine import MPSE_ERR_SHAPE
    rng = np.random.default_rng(18)
    sites = _dev(eng, _chain(rng, (1, 3, 1), (2, 2), False))
    n = 2
    ptrs = (C.c_void_p * n)(*[t.ptr for t in sites])
    codes = (C.c_int * n)(*[t.code for t in sites])
    out = (C.c_double * 2)(7.0, 7.0)
    bad_tables = ([1, 1, 2, 3, 3, 4, 3, 2, 1, 1],      # neighbours that do not match
                  [2, 1, 2, 3, 3, 3, 3, 2, 1, 1],      # first bond != 1
                  [1, 1, 2, 3, 3, 3, 3, 2, 1, 2],      # last bond != 1
                  [1, 1, 0, 3, 3, 3, 3, 2, 1, 1])      # empty physical leg
    s0, g0 = eng.mps_overlap_stats(), eng.gemm_path_stats()
    for tab in bad_tables:
        st = eng.lib.mpse_mps_overlap(eng.ctx, n, ptrs, codes, ptrs, codes, (C.c_int64 * 10)(*tab), 0, out)
        assert st == MPSE_ERR_SHAPE, (tab, st)
    assert eng.mps_overlap_stats() == s0 and eng.gemm_path_stats() == g0 and tuple(out) == (7.0, 7.0)
    with pytest.raises(ValueError):
        eng.mps_overlap(sites, sites[::-1][:1] + sites[1:], False)   # (3, 2, 1) first: not a chain
