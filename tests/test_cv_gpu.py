"""Zero-temperature correction-vector spectra (renormalizer_amd.cv.SpectraZtCV) on the GPU: the reference's recorded
spectra of its own tests, the exact resolvent of a model small enough for dense algebra, and the plumbing around
``cv_solve`` / ``batch_run``."""
import os

import numpy as np
import pytest

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity
from renormalizer_amd.utils import constant

pytestmark = pytest.mark.gpu


def _holstein_test_model():
    """renormalizer/tests/parameter.py:7-34 (3 molecules x 2 modes, 4 phonon levels), as tests/test_dmrg_gpu.py builds it"""
    omega = [Quantity(106.51, "cm^{-1}"), Quantity(1555.55, "cm^{-1}")]
    dis = [Quantity(30.1370), Quantity(8.7729)]
    ph_list = [Phonon.simple_phonon(o, d, 4) for o, d in zip(omega, dis)]
    j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
    return HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list, 15.45)] * 3, j, 3)


def _small_model(s):
    ph = Phonon.simple_phonon(Quantity(float(s["omega_cm"]), "cm^{-1}"), Quantity(float(s["displacement"])),
                              int(s["levels"]))
    jv = float(s["j_ev"])
    j = np.array([[0.0, jv], [jv, 0.0]]) / constant.au2ev
    return HolsteinModel([Mol(Quantity(float(s["elocalex_ev"]), "eV"), [ph], float(s["dipole"]))] * int(s["nmols"]), j, 3)


@pytest.mark.parametrize("method", ("1site", "2site"))
def test_zt_abs_recorded_spectrum(golden_dir, method):
    """cv/tests/test_abs.py:18-31: model, broadening, bond dimension, frequencies and tolerance are the reference's."""
    from renormalizer_amd.cv import SpectraZtCV, batch_run
    standard = np.load(os.path.join(golden_dir, "cv_abs_zt.npy"))
    freq_reg = np.arange(0.05, 0.11, 5.e-5).tolist()
    indx = [300, 680, 800, 900]
    test_freq = [freq_reg[i] for i in indx]
    standard = [v[0][0] for v in standard[indx]]
    spectra = SpectraZtCV(_holstein_test_model(), "abs", 10, 5.e-5, method=method, rtol=1e-3)
    result = batch_run(test_freq, 2, spectra)
    print(f"abs {method}: {result} recorded {standard} rel {np.abs(np.array(result) / np.array(standard) - 1)}")
    assert np.allclose(result, standard, rtol=1.e-2)


def test_zt_emi_recorded_spectrum(golden_dir):
    """cv/tests/test_emi.py:16-27 with the reference's own settings."""
    from renormalizer_amd.cv import SpectraZtCV, batch_run
    standard = np.load(os.path.join(golden_dir, "cv_emi_zt.npy"))
    freq_reg = np.arange(-0.11, -0.05, 5.e-5).tolist()
    indx = [520, 529, 661]
    standard = standard[indx]
    test_freq = [freq_reg[i] for i in indx]
    spectra = SpectraZtCV(_holstein_test_model(), "emi", 10, 5.e-5, rtol=1e-3)
    result = batch_run(test_freq, 1, spectra)
    print(f"emi: {result} recorded {standard} rel {np.abs(np.array(result) / standard - 1)}")
    assert np.allclose(result, standard, rtol=1.e-2)


@pytest.mark.parametrize("method", ("1site", "2site"))
def test_zt_abs_exact_resolvent(golden_dir, method):
    """2 molecules x 1 mode, 4 levels, m_max above every exact bond dimension: the spectrum against
    -(1/pi) Im <psi0| mu^+ (omega + e0 - H + i eta)^-1 mu |psi0> from dense algebra, at the two strongest peaks, between
    them and in both tails.  Allowed per frequency: max(3 x the deviation the reference's own SpectraZtCV showed there
    on a CPU - recorded in the fixture by tools/cv_small_reference.py; the 3 covers another random start vector and
    another number of sweeps - , the rtol of the sweep's stopping rule)."""
    from renormalizer_amd.cv import SpectraZtCV, batch_run
    s = np.load(os.path.join(golden_dir, "cv_small_exact.npz"))
    model = _small_model(s)
    eta, rtol = float(s["eta"]), float(s["rtol"])
    h = np.asarray(Mpo(model).todense())
    mu = np.asarray(Mpo.onsite(model, r"a^\dagger", dipole=True).todense())
    ew, ev = np.linalg.eigh(h)
    e0, v = ew[0], mu @ ev[:, 0]
    eye = np.eye(len(h))
    dense = np.array([-np.vdot(v, np.linalg.solve((w + e0) * eye - h + 1j * eta * eye, v)).imag / np.pi
                      for w in s["omega"]])
    # the dense values do not depend on the order of the sites: those of the fixture came from the reference's MPO
    assert np.allclose(dense, s["dense"], rtol=1e-9)
    spectra = SpectraZtCV(model, "abs", int(s["m_max"]), eta, method=method, rtol=rtol)
    assert abs(spectra.e0 - e0) < 1e-8
    result = np.array(batch_run(s["omega"].tolist(), 1, spectra))
    dev = np.abs(result - dense) / dense
    allowed = np.maximum(3 * s["reference_rel_dev"], rtol)
    print(f"exact resolvent {method}: deviation {dev} allowed {allowed} (reference {s['reference_rel_dev']})")
    assert np.all(dev <= allowed)


def test_cv_plumbing(tmp_path, monkeypatch):
    from renormalizer_amd.cv import SpectraZtCV, batch_run
    from renormalizer_amd.engine import get_engine
    from renormalizer_amd.mps.mps import Mps
    eng = get_engine()
    model = _holstein_test_model()
    first = SpectraZtCV(model, "abs", 10, 5.e-5, rtol=1e-3, procedure_cv=[0.4, 0.2, 0, 0])
    b_mps, e0 = first.b_mps, first.e0
    assert np.array_equal(np.asarray(first.cv_mps.qntot), np.asarray(b_mps.qntot))
    assert np.array_equal(np.asarray(b_mps.qntot), [1])
    start = Mps.random(model, b_mps.qntot, 10, percent=1.0, rng=np.random.default_rng(5))
    freqs = [0.0655, 0.084, 0.09]

    # passing b_mps, e0 and cv_mps skips the ground-state run (init_b_mps) and the random start (init_cv_mps): neither
    # is entered, the objects are taken as they are
    def not_called(self):
        raise AssertionError("ground state / start vector computed although b_mps, e0 and cv_mps were passed")

    def make():
        with monkeypatch.context() as m:
            m.setattr(SpectraZtCV, "init_b_mps", not_called)
            m.setattr(SpectraZtCV, "init_cv_mps", not_called)
            return _make()

    def _make():
        obj = SpectraZtCV(model, "abs", 10, 5.e-5, rtol=1e-3, procedure_cv=[0.4, 0.2, 0, 0], b_mps=b_mps, e0=e0,
                          cv_mps=start.copy())
        assert obj.b_mps is b_mps and obj.e0 == e0 and obj.procedure_gs is None
        return obj

    a = make()
    fname = str(tmp_path / "spectrum.npy")
    s0 = eng.pcg_stats()
    res = batch_run(freqs, 3, a, filename=fname)
    s1 = eng.pcg_stats()
    assert len(res) == 3 and all(isinstance(x, float) for x in res)
    assert a.batch_run and a.hop_time == [] and a.macro_iteration_result == []
    assert np.array_equal(np.load(fname), np.array(res))
    # every optimised centre is one two-layer, masked solve
    nsolve = s1["solves"] - s0["solves"]
    assert nsolve > 0 and nsolve % len(a.cv_mps) == 0
    assert s1["twolayer"] - s0["twolayer"] == nsolve and s1["masked"] - s0["masked"] == nsolve
    assert s1["end_curvature"] == s0["end_curvature"]
    assert np.array_equal(np.asarray(a.cv_mps.qntot), np.asarray(b_mps.qntot))
    assert a.cv_mps.bond_dims[0] == 1 and max(a.cv_mps.bond_dims) <= 10

    b = make()
    centres = []
    singles = []
    for w in freqs:
        t0 = eng.pcg_stats()["solves"]
        singles.append(b.cv_solve(w))
        centres.append(eng.pcg_stats()["solves"] - t0)
        assert len(b.hop_time) == centres[-1] and all(h >= 1 for h in b.hop_time)
        b.clear_res()
    assert singles == res                        # bitwise: same start, same sequence of device work
    assert sum(centres) == nsolve
