"""``cv.batch_run_lockstep`` on the GPU: the recorded spectra and the exact resolvent of tests/test_cv_gpu.py with that
file's own acceptances, the independence of a spectral value from the width and the company it runs in (bitwise), the
fallback paths and the plumbing."""
import os

import numpy as np
import pytest

from renormalizer_amd import Mpo

from test_cv_gpu import _holstein_test_model, _small_model

pytestmark = pytest.mark.gpu

ABS_FREQ = np.arange(0.05, 0.11, 5.e-5).tolist()
ABS_IDX = [300, 680, 800, 900]


@pytest.fixture(scope="module")
def abs_job():
    """b_mps and e0 of the absorption test model, computed once"""
    from renormalizer_amd.cv import SpectraZtCV
    first = SpectraZtCV(_holstein_test_model(), "abs", 10, 5.e-5, rtol=1e-3)
    return first.b_mps, first.e0


@pytest.mark.parametrize("method", ("1site", "2site"))
def test_lockstep_abs_recorded_spectrum(golden_dir, abs_job, method):
    """the frequencies, model and tolerance of test_zt_abs_recorded_spectrum; 2site runs through the fallback"""
    from renormalizer_amd.cv import SpectraZtCV, batch_run_lockstep
    from renormalizer_amd.engine import get_engine
    eng = get_engine()
    standard = np.load(os.path.join(golden_dir, "cv_abs_zt.npy"))
    standard = [v[0][0] for v in standard[ABS_IDX]]
    spectra = SpectraZtCV(_holstein_test_model(), "abs", 10, 5.e-5, method=method, rtol=1e-3, b_mps=abs_job[0],
                          e0=abs_job[1])
    s0 = eng.pcg_batch_stats()
    result = batch_run_lockstep([ABS_FREQ[i] for i in ABS_IDX], spectra, width=4)
    s1 = eng.pcg_batch_stats()
    print(f"abs {method}: {result} recorded {standard} rel {np.abs(np.array(result) / np.array(standard) - 1)}")
    assert np.allclose(result, standard, rtol=1.e-2)
    if method == "1site":
        assert s1["batched_members"] > s0["batched_members"]
    else:
        assert s1["batched_members"] == s0["batched_members"] and s1["single_members"] > s0["single_members"]


def test_lockstep_emi_recorded_spectrum(golden_dir):
    from renormalizer_amd.cv import SpectraZtCV, batch_run_lockstep
    standard = np.load(os.path.join(golden_dir, "cv_emi_zt.npy"))
    freq_reg = np.arange(-0.11, -0.05, 5.e-5).tolist()
    indx = [520, 529, 661]
    standard = standard[indx]
    spectra = SpectraZtCV(_holstein_test_model(), "emi", 10, 5.e-5, rtol=1e-3)
    result = batch_run_lockstep([freq_reg[i] for i in indx], spectra, width=3)
    print(f"emi: {result} recorded {standard} rel {np.abs(np.array(result) / standard - 1)}")
    assert np.allclose(result, standard, rtol=1.e-2)


def test_lockstep_exact_resolvent(golden_dir):
    """the acceptance of test_zt_abs_exact_resolvent: max(3 x the reference's own deviation, rtol) per frequency"""
    from renormalizer_amd.cv import SpectraZtCV, batch_run_lockstep
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
    assert np.allclose(dense, s["dense"], rtol=1e-9)
    spectra = SpectraZtCV(model, "abs", int(s["m_max"]), eta, rtol=rtol)
    result = np.array(batch_run_lockstep(s["omega"].tolist(), spectra, width=8))
    dev = np.abs(result - dense) / dense
    allowed = np.maximum(3 * s["reference_rel_dev"], rtol)
    print(f"exact resolvent lock-step: deviation {dev} allowed {allowed}")
    assert np.all(dev <= allowed)


def test_lockstep_width_and_order_bitwise(abs_job, tmp_path, monkeypatch):
    """width 1, width 3 and a shuffled list give bitwise equal values per frequency; the file is written after every
    finished frequency; the job's own correction vector is left as it was"""
    from renormalizer_amd.cv import SpectraZtCV, batch_run_lockstep
    from renormalizer_amd.engine import get_engine
    from renormalizer_amd.mps.mps import Mps
    eng = get_engine()
    model = _holstein_test_model()
    b_mps, e0 = abs_job
    start = Mps.random(model, b_mps.qntot, 10, percent=1.0, rng=np.random.default_rng(5))
    freqs = [0.0655, 0.084, 0.09, 0.0712, 0.1]

    def make():
        return SpectraZtCV(model, "abs", 10, 5.e-5, rtol=1e-3, procedure_cv=[0.4, 0.2, 0, 0], b_mps=b_mps, e0=e0,
                           cv_mps=start.copy())

    one = batch_run_lockstep(freqs, make(), width=1)
    obj = make()
    before = [np.array(a) for a in obj.cv_mps.to_arrays()]
    fname = str(tmp_path / "spectrum.npy")
    saves = []
    real_save = np.save
    monkeypatch.setattr(np, "save", lambda f, a: (saves.append(np.array(a, dtype=float)), real_save(f, a)))
    s0 = eng.pcg_batch_stats()
    three = batch_run_lockstep(freqs, obj, width=3, filename=fname)
    s1 = eng.pcg_batch_stats()
    monkeypatch.undo()
    assert s1["batched_members"] > s0["batched_members"]
    assert three == one and all(isinstance(x, float) for x in three)
    assert len(saves) == len(freqs)
    assert [int(np.isfinite(a).sum()) for a in saves] == list(range(1, len(freqs) + 1))
    assert np.array_equal(np.load(fname), np.array(three))
    after = obj.cv_mps.to_arrays()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert obj.hop_time == [] and obj.macro_iteration_result == [] and not obj.batch_run
    order = [3, 0, 4, 2, 1]
    shuffled = batch_run_lockstep([freqs[i] for i in order], make(), width=3)
    assert shuffled == [one[i] for i in order]


def test_lockstep_refuses_finite_temperature():
    from renormalizer_amd.cv import SpectraFtCV, batch_run_lockstep
    obj = SpectraFtCV.__new__(SpectraFtCV)
    with pytest.raises(NotImplementedError, match="SpectraFtCV"):
        batch_run_lockstep([0.08], obj, width=2)
