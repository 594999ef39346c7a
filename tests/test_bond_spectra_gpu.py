"""``mpse_mps_bond_spectra`` on the GPU (``Engine.mps_bond_spectra``, ``Mps.bond_spectra``, ``Mps.bond_entropies``):
the Schmidt weights p = sigma^2 of the bonds of a chain from the two environments of each bond, through the chain
kernels (``MPSE_BOND_SPECTRA_CHAIN=1``: the walks and the Jacobi eigensolver in LDS) and through the enqueued path
(``=0``: products and the block SVD); the stats say which one ran.

Reference: ``dense_spectra`` of tests/bond_spectra_refs.py, ``numpy.linalg.svd`` of the dense state reshaped at the bond
(at most 9^4 amplitudes).  Tolerances: |p - p_ref| < 1e-12 on states of norm 1 and entropies to 1e-10, the project's
tolerances for density matrices and entropies.  What to expect: an environment entry sums at most N d D products of
O(1) terms twice, and the two eigensolves are backward stable, so the weights carry a few D eps = 1e-14 at D = 64;
the NumPy restatement of the same algebra (``gram_spectra``) stays within 3e-15 of the dense SVD.  Every case prints its
largest error before it asserts."""
import os

import numpy as np
import pytest

from bond_spectra_refs import (chain_of_dense, decaying, dense_spectra, entropy, padded, scramble,
                               state_with_spectrum)          # (tests/bond_spectra_refs.py)
from chain_problems import _dev, took_path                    # (tests/chain_problems.py)

pytestmark = pytest.mark.gpu

ENV = "MPSE_BOND_SPECTRA_CHAIN"
PATHS = (("chain_kernel", "1"), ("enqueued", "0"))
SEVEN = ((1, 2, 4, 7, 4, 2, 1), 2, 2)          # bonds, d, the bond with the prescribed spectrum


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


def _rows(eng, dev, sel, path):
    """one call on the path the case means to take: the counters say that it did"""
    got, s0, s1 = took_path(eng.mps_bond_spectra_stats, lambda: eng.mps_bond_spectra(dev, sel), path, len(dev))
    assert s1["bonds"] - s0["bonds"] == len(sel) and len(got) == len(sel)
    return got


def _both_paths(eng, monkeypatch, sites, tol=1e-12, norm2=1.0, expect=None):
    """every bond through both paths against the dense SVD; ``expect``: the path either switch must end on.  Returns
    the rows of both paths."""
    ref = dense_spectra(sites)
    dev = _dev(eng, sites)
    sel = list(range(len(sites) - 1))
    out = []
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        got = _rows(eng, dev, sel, expect or path)
        dp = ds = 0.0
        for k, (g, r) in enumerate(zip(got, ref)):
            D = sites[k].shape[-1]
            assert g.shape == (D,) and g.dtype == np.float64
            assert np.all(g >= 0) and np.all(np.diff(g) <= 0)                  # clamped, descending
            dp = max(dp, np.abs(g - padded([r], D)[0]).max() / norm2)
            ds = max(ds, abs(entropy(g) - entropy(r)))
        print(f"{expect or path} bonds {[a.shape[-1] for a in sites[:-1]]}: max |dp| = {dp:.2e}, max |dS| = {ds:.2e}")
        assert dp < tol and ds < 1e-10
        out.append(got)
    monkeypatch.delenv(ENV)
    return out


PROFILES = (((1, 2, 1), 2, 0), ((1, 3, 3, 1), 3, 1), SEVEN, ((1, 4, 16, 4, 1), 4, 1), ((1, 4, 17, 4, 1), 5, 1),
            ((1, 8, 64, 8, 1), 8, 1), ((1, 9, 65, 9, 1), 9, 1))


@pytest.mark.parametrize("kind", ("real", "complex", "mixed"))
@pytest.mark.parametrize("bonds, d, cut", PROFILES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_constructed_spectra(eng, monkeypatch, bonds, d, cut, kind):
    """a prescribed spectrum, weights from 1 down to 1e-5, at the widest bond; the gauge scrambled at every bond, so
    that no environment is the identity and both solves rotate.  (1, 2, 1): one pair and no bye; (1, 3, 3, 1): a bye and
    an even pitch made odd; 16 and 17: at and one above a power of two; 64: the fit limit, all of the LDS plan; 65: one
    above, which takes the enqueued path under either switch."""
    from renormalizer_amd.engine import mps_bond_spectra_plan
    rng = np.random.default_rng(4100 + 10 * max(bonds) + ("real", "complex", "mixed").index(kind))
    ds = (d,) * (len(bonds) - 1)
    sites = state_with_spectrum(rng, bonds, ds, cut, decaying(bonds[cut + 1]), kind)
    assert abs(sum(dense_spectra(sites)[cut]) - 1) < 1e-12
    table = [[a.shape[0], a.shape[1], 1, a.shape[2]] for a in sites]
    fits = mps_bond_spectra_plan(table, len(sites) - 1, kind != "real")[1]["lds_fit_bytes"] > 0
    assert fits == (max(bonds) <= 64)
    _both_paths(eng, monkeypatch, sites, expect=None if fits else "enqueued")


def _spin_mps(sites):
    """an ``Mps`` of half spins without quantum numbers around host site tensors (D_l, 2, D_r)"""
    from renormalizer_amd import BasisHalfSpin, Model, Op
    from renormalizer_amd.mps.mps import Mps
    n = len(sites)
    ham = Op("sigma_z", 0)
    for i in range(1, n):
        ham = ham + Op("sigma_z", i)
    model = Model([BasisHalfSpin(i) for i in range(n)], ham)
    qn = [np.zeros((1, 1), dtype=int)] + [np.zeros((a.shape[-1], 1), dtype=int) for a in sites]
    return Mps.from_arrays(model, sites, qn, n - 1, np.zeros(1, dtype=int), False)


def _seven(kind="complex", seed=4200):
    bonds, d, cut = SEVEN
    return state_with_spectrum(np.random.default_rng(seed), bonds, (d,) * 6, cut, decaying(7), kind)


def test_density_operator_sites(eng, monkeypatch):
    """``MpDm.from_mps`` of the 7-bond state, then a random matrix on the ancilla leg of every site: danc = 2 and the
    ancilla leg is traced with the bonds - the spectra of the purified state"""
    from renormalizer_amd.mps.mpdm import MpDm
    rng = np.random.default_rng(4201)
    mpdm = MpDm.from_mps(_spin_mps(_seven()))
    for i in range(len(mpdm)):
        g = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
        mpdm[i] = np.einsum("apgb,gh->aphb", mpdm[i].to_host(), g)
    sites = [t.to_host() for t in mpdm]
    assert all(a.ndim == 4 and a.shape[2] == 2 for a in sites)
    ref = dense_spectra(sites)
    norm2 = float(sum(ref[0]))
    _both_paths(eng, monkeypatch, sites, norm2=norm2)
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        s0 = eng.mps_bond_spectra_stats()
        got = mpdm.bond_spectra()
        assert eng.mps_bond_spectra_stats()[path] - s0[path] == 1
        assert got.shape == (5, 7) and np.abs(got - padded(ref, 7)).max() < 1e-12 * norm2


def _degenerate_cases():
    rng = np.random.default_rng(4300)
    bell = np.zeros((2, 2, 2, 2))
    for a in range(2):
        for b in range(2):
            bell[a, b, b, a] = 0.5                                  # pairs (0, 3) and (1, 2): both cross the middle
    ghz = np.zeros((2,) * 4)
    ghz[0, 0, 0, 0] = ghz[1, 1, 1, 1] = np.sqrt(0.5)
    prod = [np.zeros((1, 2, 8)), np.zeros((8, 2, 8)), np.zeros((8, 2, 8)), np.zeros((8, 2, 1))]
    for a, v in zip(prod, ((0.6, 0.8), (1.0, 0.0), (0.8, -0.6), (0.0, 1.0))):
        a[0, :, 0] = v
    noisy = [a + 1e-16 * rng.standard_normal(a.shape) for a in prod]
    return {"bell": (scramble(rng, chain_of_dense(bell, (2,) * 4, (1, 2, 4, 2, 1)), True), {1: [0.25] * 4}),
            "ghz": (scramble(rng, chain_of_dense(ghz, (2,) * 4, (1, 2, 2, 2, 1)), False), {k: [0.5, 0.5] for k in range(3)}),
            "product": (prod, {k: [1.0] + [0.0] * 7 for k in range(3)}),
            "product_1e-16": (noisy, {k: [1.0] + [0.0] * 7 for k in range(3)})}


@pytest.mark.parametrize("name", ("bell", "ghz", "product", "product_1e-16"))
def test_degenerate_and_deficient_spectra(eng, monkeypatch, name):
    """equal weights (the rotation angle of a degenerate pair is arbitrary), exact zeros (L and M singular, the zero
    matrix threshold) and the 1e-16 padding of ``expand_bond_dimension(coef=1e-16)``, where L has eigenvalues near 1e-32"""
    sites, exact = _degenerate_cases()[name]
    for got in _both_paths(eng, monkeypatch, sites):
        for k, p in exact.items():
            assert np.abs(got[k] - np.array(p)).max() < 1e-12, (k, got[k])
        if name.startswith("product"):
            assert all(abs(entropy(g)) < 1e-12 for g in got)


def test_unnormalised_state(eng, monkeypatch):
    """norm 3: the weights sum to 9, the entropies are those of the normalised state"""
    sites = _seven("real", 4400)
    one = _both_paths(eng, monkeypatch, sites)
    sites[3] = 3.0 * sites[3]
    nine = _both_paths(eng, monkeypatch, sites, norm2=9.0)
    for a, b in zip(one, nine):
        for x, y in zip(a, b):
            assert abs(y.sum() - 9) < 1e-11 and abs(entropy(x) - entropy(y)) < 1e-12


def test_selection_and_same_bits(eng, monkeypatch):
    """a selection returns the rows of the full call bit for bit; two identical calls return identical bits"""
    dev = _dev(eng, _seven())
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        full = _rows(eng, dev, range(5), path)
        again = _rows(eng, dev, range(5), path)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(full, again))
        for sel in ((0, 3, 4), (2,), (1, 2)):
            part = _rows(eng, dev, sel, path)
            assert all(x.tobytes() == full[k].tobytes() for x, k in zip(part, sel)), (path, sel)


def test_refusals(eng, monkeypatch):
    import ctypes as C
    from renormalizer_amd.engine import MPSE_ERR_ARG, MPSE_ERR_SHAPE
    monkeypatch.delenv(ENV, raising=False)
    sites = _dev(eng, [np.ones((1, 2, 3)), np.ones((3, 2, 2)), np.ones((2, 2, 1))])
    n = 3
    ptrs = (C.c_void_p * n)(*[t.ptr for t in sites])
    codes = (C.c_int * n)(*[t.code for t in sites])
    good = [1, 2, 1, 3, 3, 2, 1, 2, 2, 2, 1, 1]
    out = (C.c_double * 5)(*([7.0] * 5))

    def call(tab=good, sel=(0, 1), o=out, nsel=None, nsite=n):
        return eng.lib.mpse_mps_bond_spectra(eng.ctx, nsite, ptrs, codes, (C.c_int64 * 12)(*tab),
                                             len(sel) if nsel is None else nsel, (C.c_int * max(len(sel), 1))(*sel), o)

    s0 = eng.mps_bond_spectra_stats()
    assert call(tab=[1, 2, 1, 3, 4, 2, 1, 2, 2, 2, 1, 1]) == MPSE_ERR_SHAPE        # neighbours that do not match
    for sel in ((1, 0), (1, 1), (0, 2), (-1, 1)):                                   # bond N - 1 is no bond
        assert call(sel=sel) == MPSE_ERR_SHAPE, sel
    assert call(sel=(), nsel=0) == MPSE_ERR_ARG
    assert call(o=None) == MPSE_ERR_ARG
    assert call(tab=[1, 2, 1, 1] + [0] * 8, sel=(0,), nsite=1) == MPSE_ERR_ARG      # one site: no bond
    assert eng.mps_bond_spectra_stats() == s0 and all(v == 7.0 for v in out)
    assert call() == 0 and all(v != 7.0 for v in out)
    for sel in ((1, 0), (1, 1), (0, 2), (-1, 1), ()):
        with pytest.raises(ValueError):
            eng.mps_bond_spectra(sites, sel)
    with pytest.raises(ValueError):
        eng.mps_bond_spectra(sites[:1], (0,))


@pytest.fixture(scope="module")
def golden(golden_dir):
    from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity
    from renormalizer_amd.mps.mps import Mps
    z = np.load(os.path.join(golden_dir, "observables_holstein_small.npz"))
    ph = [Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.274571056529368), 4),
          Phonon.simple_phonon(Quantity(3.1e-3), Quantity(9.5), 3)]
    model = HolsteinModel([Mol(Quantity(0), ph)] * 3, Quantity(3.0e-2), 3)
    n = int(z["mps_nsite"])
    mps = Mps.from_arrays(model, [z[f"mps_site_{i}"] for i in range(n)], [z[f"mps_qn_{i}"] for i in range(n + 1)],
                          int(z["mps_qnidx"]), z["mps_qntot"], bool(z["mps_to_right"]), complex(z["mps_coeff"]))
    return z, mps


def test_golden_state(eng, golden, monkeypatch):
    """the values the reference computed with its two sweeps: singular values to 1e-11 (the threshold of
    test_observables_gpu.py::test_bond_entropy; the smallest one is 0.0235), entropies to 1e-10; the state untouched"""
    z, mps = golden
    ref = z["bond_sv"]
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        s0 = eng.mps_bond_spectra_stats()
        p = mps.bond_spectra()
        s = mps.bond_entropies()
        s1 = eng.mps_bond_spectra_stats()
        assert s1[path] - s0[path] == 2 and s1["sites"] - s0["sites"] == 2 * len(mps)
        assert s1["bonds"] - s0["bonds"] == 2 * (len(mps) - 1)
        assert p.shape == (len(mps) - 1, max(mps.bond_dims))
        w = min(p.shape[1], ref.shape[1])
        assert not np.any(p[:, w:]) and not np.any(ref[:, w:])
        dsv, dent = np.abs(np.sqrt(p[:, :w]) - ref[:, :w]).max(), np.abs(s - z["bond_entropy"]).max()
        print(f"{path}: max |sqrt(p) - bond_sv| = {dsv:.2e}, max |S - bond_entropy| = {dent:.2e}")
        assert dsv < 1e-11 and dent < 1e-10
        one = mps.bond_spectra(3)
        assert one.shape == (1, mps.bond_dims[4]) and one[0].tobytes() == p[3, :one.shape[1]].tobytes()
    assert np.abs(np.asarray(mps.e_occupations) - z["e_occupations"]).max() < 1e-12


def test_entropies_against_the_sweeps(eng, golden, monkeypatch):
    """``bond_entropies()`` against ``calc_entropy("bond")``, the copy and the two sweeps, on the golden state and on
    the 7-bond state"""
    for mps in (golden[1], _spin_mps(_seven())):
        ref = mps.calc_entropy("bond")
        for path, env in PATHS:
            monkeypatch.setenv(ENV, env)
            got = mps.bond_entropies()
            print(f"{path}: max |bond_entropies - calc_entropy| = {np.abs(got - ref).max():.2e}")
            assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-10


def test_gauge_independence(eng, golden, monkeypatch):
    mps = golden[1]
    other = mps.copy()
    other.ensure_left_canonical()
    assert other.check_left_canonical()
    for path, env in PATHS:
        monkeypatch.setenv(ENV, env)
        assert np.abs(mps.bond_spectra() - other.bond_spectra()).max() < 1e-12


def test_sweep_counter_after_the_whole_file(eng):
    """last in the file: the largest sweep count of any Jacobi solve so far is at most half the cap, which therefore
    is the safety condition it is meant to be"""
    from renormalizer_amd.engine import mps_bond_spectra_plan
    cap = mps_bond_spectra_plan([[1, 2, 1, 2], [2, 2, 1, 1]], 1, False)[1]["sweep_cap"]
    _rows(eng, _dev(eng, _seven()), range(5), "chain_kernel")     # (run on its own, the test still has a solve behind it)
    top = eng.mps_bond_spectra_stats()["max_sweeps"]
    print(f"largest sweep count {top}, cap {cap}")
    assert 1 <= top <= cap // 2
