"""``Mps.site_rdms`` / ``site_expectations`` / ``occupations`` / ``site_entropies`` on the GPU: the one-call siblings of
``calc_1site_rdm``, ``expectations``, ``e_occupations`` + ``ph_occupations`` and ``calc_entropy("1site")``, against the
values the real reference computed for a fixed complex MPS (tests/golden/observables_holstein_small.npz) and against
the existing methods.  The golden state has norm 1, 9 sites and small bonds: the rounding bound of
tests/test_rdm1_gpu.py gives about 1e-13, the tolerance is the 1e-12 ``calc_1site_rdm`` is held to."""
import os

import numpy as np
import pytest

from renormalizer_amd import HolsteinModel, Mol, Mpo, Op, Phonon, Quantity

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
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


def _calls(stats):
    return stats["chain_kernel"] + stats["enqueued"]


def test_reference_values(state, eng):
    z, mps = state
    n = len(mps)
    rdm = mps.site_rdms()
    assert sorted(rdm) == list(range(n))
    err = max(np.abs(rdm[k] - z[f"rdm1_{k}"]).max() for k in range(n))
    print(f"max |site_rdms - reference| = {err:.2e}")
    for k, v in rdm.items():
        assert v.shape == z[f"rdm1_{k}"].shape and v.dtype == np.complex128
        assert np.abs(v - z[f"rdm1_{k}"]).max() < 1e-12
    assert set(mps.site_rdms([2, 5])) == {2, 5} and set(mps.site_rdms(4)) == {4}
    s0 = eng.mps_rdm1_stats()
    e_occ, ph_occ = mps.occupations()
    s1 = eng.mps_rdm1_stats()
    # one engine call over the distinct sites of the electronic and the vibrational dofs
    dofs = list(mps.model.e_dofs) + list(mps.model.v_dofs)
    assert _calls(s1) - _calls(s0) == 1
    assert s1["matrices"] - s0["matrices"] == len({mps.model.dof_to_siteidx[d] for d in dofs})
    print(f"max |occupations - reference| = {np.abs(e_occ - z['e_occupations']).max():.2e} (electrons), "
          f"{np.abs(ph_occ - z['ph_occupations']).max():.2e} (phonons)")
    assert e_occ.dtype == np.float64 and ph_occ.dtype == np.float64
    assert np.abs(e_occ - z["e_occupations"]).max() < 1e-12
    assert np.abs(ph_occ - z["ph_occupations"]).max() < 1e-12
    s = mps.site_entropies()
    assert sorted(s) == list(range(n))
    assert np.abs(np.array([s[k] for k in range(n)]) - z["site_entropy"]).max() < 1e-10


def test_operators(state):
    z, mps = state
    model = mps.model
    for sym, dofs in (("n", model.v_dofs), (r"a^\dagger a", model.e_dofs), ("x", model.v_dofs)):
        got = mps.site_expectations(sym, dofs)
        ref = mps.expectations([Mpo(model, Op(sym, dof)) for dof in dofs])
        err = np.abs(got - ref).max()
        print(f"{sym}: max |site_expectations - expectations| = {err:.2e}, largest value {np.abs(ref).max():.2e}")
        assert got.shape == (len(dofs),) and err < 1e-12
    assert np.abs(mps.site_expectations("x", model.v_dofs)).max() > 1e-3          # not a comparison of zeros
    with pytest.raises(ValueError):
        mps.site_expectations(r"a^\dagger a", [[model.e_dofs[0], model.e_dofs[1]]])
    with pytest.raises(ValueError):
        mps.site_expectations("n", ["no such dof"])


def test_several_dofs_on_one_site(eng):
    from renormalizer_amd.mps.mps import Mps
    ph = Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.27), 3)
    model = HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(3.0e-2), 4)
    assert len({model.dof_to_siteidx[d] for d in model.e_dofs}) == 1 and len(model.e_dofs) == 3
    mps = Mps.random(model, 1, 6, rng=np.random.default_rng(41)).to_complex()
    for i in range(len(mps)):           # a complex state: random phases on every site
        a = mps[i].to_host()
        mps[i] = a * np.exp(1j * np.random.default_rng(42 + i).uniform(0, 2 * np.pi, a.shape))
    mps.canonicalise().normalize("mps_only")
    s0 = eng.mps_rdm1_stats()
    e_occ, ph_occ = mps.occupations()
    s1 = eng.mps_rdm1_stats()
    assert _calls(s1) - _calls(s0) == 1 and s1["matrices"] - s0["matrices"] == 1 + len(model.v_dofs)
    ref = np.asarray(mps.e_occupations)
    print(f"scheme 4: max |occupations - e_occupations| = {np.abs(e_occ - ref).max():.2e}")
    assert np.abs(e_occ - ref).max() < 1e-12 and abs(e_occ.sum() - 1) < 1e-12
    assert np.abs(ph_occ - np.asarray(mps.ph_occupations)).max() < 1e-12


def test_density_operator():
    """a cooled MpDm of a small Holstein dimer, built as in tests/test_mpdm_gpu.py (reduced density matrices of a
    density operator): 4-leg sites, the ancilla leg traced"""
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
    ref = rho.calc_1site_rdm()
    top = max(np.abs(v).max() for v in ref.values())
    got = rho.site_rdms()
    assert sorted(got) == sorted(ref)
    err = max(np.abs(got[k] - ref[k]).max() for k in ref)
    print(f"MpDm: max |site_rdms - calc_1site_rdm| / max|rdm| = {err / top:.2e}")
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype
        assert np.abs(got[k] - ref[k]).max() <= 1e-12 * top
    only = rho.site_rdms(idx=[1, 3])
    assert sorted(only) == [1, 3]
    for k in only:
        assert np.abs(only[k] - ref[k]).max() <= 1e-12 * top


def test_nothing_old_moved(state):
    z, mps = state
    before = (np.asarray(mps.e_occupations).tobytes(), np.asarray(mps.ph_occupations).tobytes(),
              {k: v.tobytes() for k, v in mps.calc_1site_rdm().items()})
    mps.site_rdms()
    mps.occupations()
    after = (np.asarray(mps.e_occupations).tobytes(), np.asarray(mps.ph_occupations).tobytes(),
             {k: v.tobytes() for k, v in mps.calc_1site_rdm().items()})
    assert before == after
