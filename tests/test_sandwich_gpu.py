"""``mpse_mps_sandwich`` on the GPU (``Engine.mps_sandwich`` / ``Mps.matrix_element``): chains of numpy arrays from a
fixed seed against the same contraction with ``np.einsum`` on the host, and against ``Mps.expectation`` where an ``Mpo``
is at hand.

Tolerance: 4 * 2^-53 * (sum_i n_i) * prod_i |B_i|_F |W_i|_F |K_i|_F with n_i = Dbl Dkl wl d^2 danc, the number of
products summed into one entry of E_{i+1}: the standard bound of an inner product of n terms, n u |x| |y|, carried
through the chain with |E_{i+1}|_F <= |B_i|_F |W_i|_F |E_i|_F |K_i|_F, and a factor 4 for complex arithmetic.  Every
case prints error / scale before it asserts, and asserts through ``mps_sandwich_stats`` that it took the path it means
to take."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from chain_problems import _chain, _dev, _mpo, took_path   # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_sandwich(bra, w, ket, conj_bra):
    e = np.ones((1, 1, 1))
    for b, m, k in zip(bra, w, ket):
        b4 = b if b.ndim == 4 else b[:, :, None, :]
        k4 = k if k.ndim == 4 else k[:, :, None, :]
        if conj_bra:
            b4 = b4.conj()
        e = np.einsum("bsac,gstf,bgk,ktal->cfl", b4, m, e, k4, optimize=True)
    return complex(e[0, 0, 0])


def _scale(bra, w, ket):
    return float(np.prod([np.linalg.norm(b) * np.linalg.norm(m) * np.linalg.norm(k) for b, m, k in zip(bra, w, ket)]))


def _tol(bra, w, ket):
    n = 0
    for b, m, k in zip(bra, w, ket):
        danc = b.shape[2] if b.ndim == 4 else 1
        n += b.shape[0] * k.shape[0] * m.shape[0] * b.shape[1] ** 2 * danc
    return 4.0 * 2.0 ** -53 * n * _scale(bra, w, ket)


def _run(eng, bra, w, ket, conj_bra, path):
    """one call on the path the case means to take (asserted through the stats); returns the value"""
    return took_path(eng.mps_sandwich_stats,
                     lambda: eng.mps_sandwich(_dev(eng, bra), _dev(eng, w), _dev(eng, ket), conj_bra), path, len(bra))[0]


def _check(eng, bra, w, ket, conj_bra, path, label=""):
    got = _run(eng, bra, w, ket, conj_bra, path)
    ref, tol, scale = _host_sandwich(bra, w, ket, conj_bra), _tol(bra, w, ket), _scale(bra, w, ket)
    print(f"{label or path}: |sandwich - einsum| / scale = {abs(got - ref) / scale:.2e} (tolerance {tol / scale:.2e})")
    assert abs(got - ref) <= tol, (got, ref, tol)
    return got


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


BRA5, KET5, W5, D5 = (1, 2, 5, 3, 2, 1), (1, 3, 4, 4, 3, 1), (1, 3, 5, 2, 4, 1), (2, 3, 2, 3, 2)


def test_single_site(eng):
    rng = np.random.default_rng(21)
    for cplx in (False, True):
        bra, ket, w = _chain(rng, (1, 1), (3,), cplx), _chain(rng, (1, 1), (3,), cplx), _mpo(rng, (1, 1), (3,), cplx)
        for conj_bra in (False, True):
            _check(eng, bra, w, ket, conj_bra, "chain_kernel", f"single site complex={cplx}")


@pytest.mark.parametrize("kind", ("real", "complex", "mixed"))
def test_rectangular_chain(eng, kind):
    """bra bonds != ket bonds != MPO bonds, no power of two, d alternating 2 / 3; mixed: a real bra, a ket complex only
    at sites 2 - 3 and a W complex at one site"""
    rng = np.random.default_rng(22)
    bra_c = {"real": False, "complex": True, "mixed": False}[kind]
    ket_c = {"real": False, "complex": True, "mixed": [False, False, True, True, False]}[kind]
    w_c = {"real": False, "complex": True, "mixed": [False, True, False, False, False]}[kind]
    bra, ket, w = _chain(rng, BRA5, D5, bra_c), _chain(rng, KET5, D5, ket_c), _mpo(rng, W5, D5, w_c)
    for conj_bra in (False, True):
        _check(eng, bra, w, ket, conj_bra, "chain_kernel", f"{kind} conj_bra={conj_bra}")


def test_mixed_chain_through_the_enqueued_updates(eng, monkeypatch):
    """the mixed chain of test_rectangular_chain with the kernel switched off (the switch is read per call): the real
    bra and the real ket sites next to complex operands are widened into pooled complex copies on the way"""
    rng = np.random.default_rng(22)
    bra, ket = _chain(rng, BRA5, D5, False), _chain(rng, KET5, D5, [False, False, True, True, False])
    w = _mpo(rng, W5, D5, [False, True, False, False, False])
    for conj_bra in (False, True):
        kernel = _run(eng, bra, w, ket, conj_bra, "chain_kernel")
        monkeypatch.setenv("MPSE_SANDWICH_CHAIN", "0")
        enq = _check(eng, bra, w, ket, conj_bra, "enqueued", f"mixed enqueued conj_bra={conj_bra}")
        monkeypatch.delenv("MPSE_SANDWICH_CHAIN")
        print(f"|chain - enqueued| / scale = {abs(kernel - enq) / _scale(bra, w, ket):.2e}")
        assert abs(kernel - enq) <= 2 * _tol(bra, w, ket)


def test_conjugation_differs_on_complex_data(eng):
    rng = np.random.default_rng(23)
    bra, ket, w = _chain(rng, BRA5, D5, True), _chain(rng, KET5, D5, True), _mpo(rng, W5, D5, True)
    plain = _check(eng, bra, w, ket, False, "chain_kernel", "plain")
    conj = _check(eng, bra, w, ket, True, "chain_kernel", "conjugated")
    assert abs(plain - conj) > 2 * _tol(bra, w, ket)
    # a bra that is complex at some sites only is conjugated site by site
    bra_m = _chain(rng, BRA5, D5, [True, False, True, False, False])
    a, b = _check(eng, bra_m, w, ket, False, "chain_kernel"), _check(eng, bra_m, w, ket, True, "chain_kernel")
    assert abs(a - b) > 2 * _tol(bra_m, w, ket)


@pytest.mark.parametrize("d", (2, 3))
def test_density_operator_sites(eng, d):
    rng = np.random.default_rng(24)
    bra = _chain(rng, (1, 3, 5, 1), (d,) * 3, True, danc=(d,) * 3)
    ket = _chain(rng, (1, 4, 2, 1), (d,) * 3, [False, True, False], danc=(d,) * 3)
    w = _mpo(rng, (1, 3, 2, 1), (d,) * 3, False)
    for conj_bra in (False, True):
        _check(eng, bra, w, ket, conj_bra, "chain_kernel", f"density operator d={d} conj_bra={conj_bra}")


def test_structural_zeros_are_skipped_exactly(eng):
    """a lower-triangular channel pattern and one all-zero channel: the value matches, and it matches the run in which
    the zeros are 1e-300 (entries the kernel then multiplies by) to the tolerance"""
    rng = np.random.default_rng(25)
    wb = (1, 4, 4, 4, 1)
    bra, ket = _chain(rng, (1, 3, 6, 3, 1), (2, 3, 2, 3), True), _chain(rng, (1, 4, 5, 4, 1), (2, 3, 2, 3), True)
    w = _mpo(rng, wb, (2, 3, 2, 3), False)
    for m in w[1:3]:
        for g in range(m.shape[0]):
            m[g, :, :, g + 1:] = 0.0        # channel g feeds channels <= g only
    w[1][:, :, :, 2] = 0.0                  # nothing reaches channel 2 of bond 2
    w[0][0, 0, 1, :] = 0.0                  # and single entries
    w[3][1, 2, 0, 0] = 0.0
    assert sum(int((m == 0).sum()) for m in w) > 40
    a = _check(eng, bra, w, ket, True, "chain_kernel", "structural zeros")
    w_tiny = [np.where(m == 0, 1e-300, m) for m in w]
    b = _check(eng, bra, w_tiny, ket, True, "chain_kernel", "zeros as 1e-300")
    print(f"|zeros - tiny| / scale = {abs(a - b) / _scale(bra, w, ket):.2e}")
    assert abs(a - b) <= _tol(bra, w, ket)


def test_identity_mpo_is_the_overlap(eng):
    from renormalizer_amd.mps.mps import Mps
    rng = np.random.default_rng(26)
    bra, ket = _chain(rng, BRA5, D5, True), _chain(rng, KET5, D5, [False, True, True, False, True])
    w = [np.eye(d).reshape(1, d, d, 1) for d in D5]
    mb, mk = Mps(), Mps()
    mb._mp, mk._mp = _dev(eng, bra), _dev(eng, ket)
    for conj_bra in (False, True):
        val = _check(eng, bra, w, ket, conj_bra, "chain_kernel", "identity MPO")
        ov = mb.overlap(mk, self_is_conj=not conj_bra)
        print(f"|sandwich - overlap| / scale = {abs(val - ov) / _scale(bra, w, ket):.2e}")
        assert abs(val - ov) <= _tol(bra, w, ket)


def _limit_chain(rng, extra_channels=0):
    """the complex two-site chain of tests/test_sandwich_host.py whose launch is exactly the LDS budget (read from the
    plan), normalised site by site"""
    from renormalizer_amd.engine import mps_sandwich_plan
    budget = mps_sandwich_plan([[1] * 8], True)[1]["lds_budget"]
    k, wch = 3, 5
    a = budget // (16 * wch * (k + 1))
    bra, ket = _chain(rng, (1, a, 1), (2, 2), True), _chain(rng, (1, k, 1), (2, 2), True)
    w = _mpo(rng, (1, wch + extra_channels, 1), (2, 2), False)
    return [[x / np.linalg.norm(x) for x in t] for t in (bra, w, ket)], budget


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_sandwich_gpu as t
from renormalizer_amd.engine import get_engine
eng = get_engine()
(bra, w, ket), _ = t._limit_chain(np.random.default_rng(27))
val = t._run(eng, bra, w, ket, True, "enqueued")
print("VALUE", val.real.hex(), val.imag.hex())
"""


def test_lds_limit_and_above(eng):
    from renormalizer_amd.engine import mps_sandwich_plan
    (bra, w, ket), budget = _limit_chain(np.random.default_rng(27))
    ok, info = mps_sandwich_plan(eng.sandwich_dims(_dev(eng, bra), _dev(eng, w), _dev(eng, ket)), True)
    assert ok and info["lds_bytes"] == budget
    at_limit = _check(eng, bra, w, ket, True, "chain_kernel", "at the LDS limit")
    (bra1, w1, ket1), _ = _limit_chain(np.random.default_rng(28), extra_channels=1)
    ok1, info1 = mps_sandwich_plan(eng.sandwich_dims(_dev(eng, bra1), _dev(eng, w1), _dev(eng, ket1)), True)
    assert not ok1 and info1["valid"] == 1
    _check(eng, bra1, w1, ket1, True, "enqueued", "one channel above the limit")
    # the chain at the limit through the enqueued updates: the variable is read at call time, in a fresh process
    env = dict(os.environ, MPSE_SANDWICH_CHAIN="0")
    res = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    line = [x for x in res.stdout.splitlines() if x.startswith("VALUE")][0].split()
    other = complex(float.fromhex(line[1]), float.fromhex(line[2]))
    print(f"|chain - enqueued| / scale = {abs(at_limit - other) / _scale(bra, w, ket):.2e}")
    assert abs(at_limit - other) <= _tol(bra, w, ket)
    assert abs(other - _host_sandwich(bra, w, ket, True)) <= _tol(bra, w, ket)


def _holstein():
    from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity
    ph = Phonon.simple_phonon(Quantity(1), Quantity(1), 2)
    return HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(1), 3)


def test_model_states(eng):
    from renormalizer_amd import Mpo
    from renormalizer_amd.mps.mpdm import MpDm
    from renormalizer_amd.mps.mps import Mps
    model = _holstein()
    mpo = Mpo(model)
    mps = Mps.random(model, 1, 8, rng=np.random.default_rng(29))
    mps.canonicalise()
    mps.normalize("mps_only")
    mpdm = MpDm.max_entangled_ex(model)
    for name, state in (("Mps", mps), ("MpDm", mpdm)):
        s0 = eng.mps_sandwich_stats()
        val = state.matrix_element(mpo, state, self_is_conj=False)
        s1 = eng.mps_sandwich_stats()
        ref = state.expectation(mpo)
        print(f"{name}: matrix_element {val!r}, expectation {ref!r}, relative difference {abs(val - ref) / abs(ref):.2e}")
        assert s1["chain_kernel"] == s0["chain_kernel"] + 1 and s1["sites"] == s0["sites"] + len(state)
        assert abs(ref) > 1e-3 and abs(val - ref) <= 1e-12 * abs(ref)
    # Op / OpSum are accepted like expectation does
    from renormalizer_amd.model.op import Op
    op = Op(r"a^\dagger a", 1)
    assert abs(mps.matrix_element(op, mps, self_is_conj=False) - mps.expectation(op)) <= 1e-12


def test_same_inputs_same_bits(eng):
    from renormalizer_amd.engine import mps_sandwich_plan
    rng = np.random.default_rng(30)
    wide = mps_sandwich_plan([[1] * 8], True)[1]["channel_limit"] + 1
    cases = (("chain_kernel", BRA5, KET5, W5), ("enqueued", BRA5, KET5, (1, 3, wide, 2, 4, 1)))
    for path, bb, kb, wb in cases:
        bra, ket, w = _chain(rng, bb, D5, True), _chain(rng, kb, D5, True), _mpo(rng, wb, D5, False)
        a, b = _check(eng, bra, w, ket, False, path), _run(eng, bra, w, ket, False, path)
        assert a.real.hex() == b.real.hex() and a.imag.hex() == b.imag.hex()


def test_bad_tables_are_refused_without_device_work(eng):
    from renormalizer_amd.engine import MPSE_ERR_ARG, MPSE_ERR_SHAPE
    rng = np.random.default_rng(31)
    sites = _dev(eng, _chain(rng, (1, 3, 1), (2, 2), False))
    ws = _dev(eng, _mpo(rng, (1, 2, 1), (2, 2), False))
    n = 2
    ptrs = (C.c_void_p * n)(*[t.ptr for t in sites])
    wptrs = (C.c_void_p * n)(*[t.ptr for t in ws])
    codes = (C.c_int * n)(*[t.code for t in sites])
    out = (C.c_double * 2)(7.0, 7.0)
    good = [1, 1, 1, 2, 1, 3, 3, 2, 3, 3, 2, 2, 1, 1, 1, 1]

    def call(tab, w_codes=codes):
        return eng.lib.mpse_mps_sandwich(eng.ctx, n, ptrs, codes, ptrs, codes, wptrs, w_codes, (C.c_int64 * 16)(*tab), 0, out)

    def bad(pos, val):
        t = list(good)
        t[pos] = val
        return t

    s0, g0 = eng.mps_sandwich_stats(), eng.gemm_path_stats()
    for tab in (bad(8, 4), bad(9, 2), bad(10, 3), bad(0, 2), bad(2, 2), bad(14, 2), bad(15, 2), bad(3, 0), bad(12, 0)):
        assert call(tab) == MPSE_ERR_SHAPE, tab
    assert call(good, (C.c_int * n)(0, 7)) == MPSE_ERR_ARG
    assert eng.lib.mpse_mps_sandwich(eng.ctx, n, ptrs, codes, ptrs, codes, None, codes, (C.c_int64 * 16)(*good), 0,
                                     out) == MPSE_ERR_ARG
    assert eng.mps_sandwich_stats() == s0 and eng.gemm_path_stats() == g0 and tuple(out) == (7.0, 7.0)
    assert call(good) == 0 and tuple(out) != (7.0, 7.0)
    with pytest.raises(ValueError):
        eng.mps_sandwich(sites, ws[:1], sites, False)
