"""``Mps.pair_rdms`` / ``pair_entropies`` / ``mutual_information`` on the GPU: the one-call siblings of
``calc_2site_rdm``, ``calc_entropy("2site")`` and ``calc_entropy("mutual")``, against the values the real reference
computed for a fixed complex MPS (tests/golden/observables_holstein_small.npz, the state of
tests/test_site_rdms_gpu.py) and against the existing methods.  The golden state has norm 1, 9 sites and small bonds:
the rounding bound of tests/test_rdm2_gpu.py gives about 1e-13, the tolerance is the 1e-12 ``calc_2site_rdm`` is held
to (tests/test_observables_gpu.py)."""
import os

import numpy as np
import pytest

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def state(golden_dir):
    from renormalizer_amd.mps.mps import Mps
    z = np.load(os.path.join(golden_dir, "observables_holstein_small.npz"))
    ph = [Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.274571056529368), 4),
          Phonon.simple_phonon(Quantity(3.1e-3), Quantity(9.5), 3)]
    model = HolsteinModel([Mol(Quantity(0), ph)] * 3, Quantity(3.0e-2), 3)
    n = int(z["mps_nsite"])
    assert n == model.nsite
    mps = Mps.from_arrays(model, [z[f"mps_site_{i}"] for i in range(n)], [z[f"mps_qn_{i}"] for i in range(n + 1)],
                          int(z["mps_qnidx"]), z["mps_qntot"], bool(z["mps_to_right"]), complex(z["mps_coeff"]))
    return z, mps


@pytest.fixture(scope="module")
def old_pairs(state):
    """``calc_2site_rdm()`` of the golden state, computed once"""
    return state[1].calc_2site_rdm()


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


def _calls(stats):
    return stats["chain_kernel"] + stats["enqueued"]


def test_reference_values(state, eng):
    z, mps = state
    n = len(mps)
    s0 = eng.mps_rdm2_stats()
    rdm = mps.pair_rdms()
    s1 = eng.mps_rdm2_stats()
    assert _calls(s1) - _calls(s0) == 1 and s1["pairs"] - s0["pairs"] == 36       # one call for the whole chain
    assert sorted(rdm) == [(i, j) for i in range(n) for j in range(i + 1, n)] and len(rdm) == 36
    recorded = ((0, 1), (0, 4), (2, 3), (3, 8), (7, 8))
    err = max(np.abs(rdm[ij] - z["rdm2_%d_%d" % ij]).max() for ij in recorded)
    print(f"max |pair_rdms - reference| = {err:.2e}")
    for ij in recorded:
        ref = z["rdm2_%d_%d" % ij]
        assert rdm[ij].shape == ref.shape and rdm[ij].dtype == np.complex128
        assert np.abs(rdm[ij] - ref).max() < 1e-12
    s2 = mps.pair_entropies()
    assert sorted(s2) == sorted(rdm)
    err = max(abs(s2[(int(i), int(j))] - v) for i, j, v in z["pair_entropy"])
    print(f"max |pair_entropies - reference| = {err:.2e}")
    assert len(z["pair_entropy"]) == 36 and err < 1e-9
    r0, p0 = eng.mps_rdm1_stats(), eng.mps_rdm2_stats()
    mi = mps.mutual_information()
    r1, p1 = eng.mps_rdm1_stats(), eng.mps_rdm2_stats()
    assert _calls(r1) - _calls(r0) == 1 and _calls(p1) - _calls(p0) == 1          # one call of each kind
    print(f"max |mutual_information - reference| = {np.abs(mi - z['mutual_entropy']).max():.2e}")
    assert mi.shape == z["mutual_entropy"].shape == (n, n) and mi.dtype == np.float64
    assert np.abs(mi - z["mutual_entropy"]).max() < 1e-9


def test_against_calc_2site_rdm(state, old_pairs):
    _, mps = state
    new = mps.pair_rdms()
    assert sorted(new) == sorted(old_pairs)
    err = max(np.abs(new[k] - old_pairs[k]).max() for k in old_pairs)
    print(f"max |pair_rdms - calc_2site_rdm| = {err:.2e}")
    for k, v in old_pairs.items():
        assert new[k].shape == v.shape and new[k].dtype == v.dtype
        assert np.abs(new[k] - v).max() < 1e-12


def test_selections(state, old_pairs, eng):
    _, mps = state
    some = mps.pair_rdms([2, 5, 7])
    assert sorted(some) == [(2, 5), (2, 7), (5, 7)]
    for k, v in some.items():
        assert np.abs(v - old_pairs[k]).max() < 1e-12
    assert sorted(mps.pair_rdms([7, 2, 2])) == [(2, 7)]                   # any order, repeated sites count once
    s0 = eng.mps_rdm2_stats()
    assert mps.pair_rdms([4]) == {} and mps.pair_rdms([]) == {} and mps.pair_entropies([4]) == {}
    assert mps.mutual_information([4]).shape == (1, 1)
    assert eng.mps_rdm2_stats() == s0                                     # no engine call for fewer than two sites
    mi = mps.mutual_information([2, 5, 7])
    full = mps.mutual_information()
    assert mi.shape == (3, 3) and np.abs(mi - full[np.ix_([2, 5, 7], [2, 5, 7])]).max() < 1e-12


def test_real_state():
    from renormalizer_amd.mps.mps import Mps
    ph = Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.27), 3)
    model = HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(3.0e-2), 3)
    mps = Mps.random(model, 1, 6, rng=np.random.default_rng(41))
    mps.canonicalise().normalize("mps_only")
    assert not mps.is_complex
    ref = mps.calc_2site_rdm()
    got = mps.pair_rdms()
    assert sorted(got) == sorted(ref)
    for k, v in ref.items():
        assert got[k].dtype == np.float64 == v.dtype and got[k].shape == v.shape
        assert np.abs(got[k] - v).max() < 1e-12


def test_density_operator():
    """a cooled MpDm of a small Holstein dimer, built as in tests/test_site_rdms_gpu.py::test_density_operator: 4-leg
    sites, the ancilla leg traced"""
    from renormalizer_amd.mps import MpDm, thermal_state
    from renormalizer_amd.utils import CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, constant
    ph = [Phonon.simple_phonon(Quantity(1555.55, "cm^{-1}"), Quantity(8.7729), 3)]
    j = np.array([[0.0, -0.1], [-0.1, 0.0]]) / constant.au2ev
    model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph, 15.45)] * 2, j, 3)
    init = MpDm.max_entangled_ex(model)
    init.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=8)
    init.evolve_config = EvolveConfig(EvolveMethod.tdvp_ps, adaptive=False, guess_dt=0.1 / 1j)
    beta = Quantity(298, "K").to_beta()
    rho, _ = thermal_state(init, Mpo(model), beta / 2j / 4, 4, auto_expand=True)
    assert all(t.ndim == 4 for t in rho)
    ref = rho.calc_2site_rdm()
    top = max(np.abs(v).max() for v in ref.values())
    got = rho.pair_rdms()
    assert sorted(got) == sorted(ref)
    err = max(np.abs(got[k] - ref[k]).max() for k in ref)
    print(f"MpDm: max |pair_rdms - calc_2site_rdm| / max|rdm| = {err / top:.2e}")
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype
        assert np.abs(got[k] - ref[k]).max() <= 1e-12 * top


def test_nothing_old_moved(state, old_pairs):
    _, mps = state
    before = {k: v.tobytes() for k, v in old_pairs.items()}
    mps.pair_rdms()
    mps.pair_entropies([0, 3])
    mps.mutual_information()
    after = {k: v.tobytes() for k, v in mps.calc_2site_rdm().items()}
    assert before == after
