"""Time-domain spectra (renormalizer_amd.spectra) on the GPU against the series recorded by the reference's own
spectra/tests/test_spectra.py: the same model, dt = 30, offsets, configurations and acceptances
(``np.allclose(rtol=1e-2)``, the exact emission 1e-3), over a prefix of each series so that every case takes seconds."""
import os

import numpy as np
import pytest

from renormalizer_amd import OptimizeConfig, Quantity

from test_cv_gpu import _holstein_test_model

pytestmark = pytest.mark.gpu

DT = 30.0


def _offset(model):
    """renormalizer/tests/parameter.py:32"""
    return Quantity(2.28614053, "ev") + Quantity(model.gs_zpe)


def _std(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"spectra_{name}.npy"))


def _compare(name, got, std, rtol):
    n = len(got)
    dev = np.abs(got - std[:n]) / np.abs(std[:n])
    print(f"{name}: {n} values, max relative deviation from the recorded series {dev.max():.2e}")
    assert np.allclose(got, std[:n], rtol=rtol)


def test_zero_exact_emi(golden_dir):
    from renormalizer_amd.spectra import SpectraExact
    job = SpectraExact(_holstein_test_model(), "emi", rng=np.random.default_rng(0))
    job.info_interval = 100
    job.evolve(DT, 300)
    _compare("exact emi", job.autocorr[:300], _std(golden_dir, "ZeroExactEmi"), 1e-3)


@pytest.mark.parametrize("algorithm", (1, 2))
def test_zero_t_abs(golden_dir, algorithm):
    from renormalizer_amd.spectra import SpectraOneWayPropZeroT, SpectraTwoWayPropZeroT
    cls = SpectraOneWayPropZeroT if algorithm == 1 else SpectraTwoWayPropZeroT
    model = _holstein_test_model()
    job = cls(model.switch_scheme(2), "abs", OptimizeConfig(procedure=[[1, 0], [1, 0], [1, 0]]), offset=_offset(model),
              rng=np.random.default_rng(0))
    job.info_interval = 30
    job.evolve(DT, 40)
    _compare(f"zero-T abs {algorithm}", job.autocorr[:40], _std(golden_dir, f"ZeroTabs_{algorithm}svd"), 1e-2)


@pytest.mark.parametrize("algorithm", (1, 2))
def test_zero_t_emi(golden_dir, algorithm):
    from renormalizer_amd.spectra import SpectraOneWayPropZeroT, SpectraTwoWayPropZeroT
    cls = SpectraOneWayPropZeroT if algorithm == 1 else SpectraTwoWayPropZeroT
    model = _holstein_test_model()
    # the recorded series carries the offset 2.28614053 eV already: only the zero-point energy is taken out
    job = cls(model, "emi", offset=Quantity(model.gs_zpe), rng=np.random.default_rng(0))
    job.info_interval = 50
    job.evolve(DT, 40)
    _compare(f"zero-T emi {algorithm}", job.autocorr[:40], _std(golden_dir, "ZeroExactEmi"), 1e-2)


def test_finite_t_abs(golden_dir):
    from renormalizer_amd.spectra import SpectraFiniteT
    model = _holstein_test_model()
    job = SpectraFiniteT(model, "abs", Quantity(298, "K"), 50, _offset(model))
    job.evolve(DT, 20)
    _compare("finite-T abs", job.autocorr[:20], _std(golden_dir, "TTabs_svd"), 1e-2)


@pytest.fixture(scope="module")
def emi_runs(tmp_path_factory):
    """finite-temperature emission twice under one dump_dir / job_name: the second job reads the thermal state back"""
    from renormalizer_amd.spectra import SpectraFiniteT
    dump_dir = str(tmp_path_factory.mktemp("spectra_emi"))
    model = _holstein_test_model()
    jobs = []
    for _ in range(2):
        job = SpectraFiniteT(model, "emi", Quantity(298, "K"), 50, _offset(model), dump_dir=dump_dir, job_name="emi")
        job.evolve(DT, 15)
        jobs.append(job)
    return dump_dir, jobs


def test_finite_t_emi(golden_dir, emi_runs):
    _compare("finite-T emi", emi_runs[1][0].autocorr[:15], _std(golden_dir, "TTemi_2svd"), 1e-2)


def test_finite_t_emi_reads_the_thermal_state_back(emi_runs):
    dump_dir, (first, second) = emi_runs
    assert os.path.exists(os.path.join(dump_dir, "emi_impo.npz"))
    assert not first.thermal_state_loaded and second.thermal_state_loaded
    assert len(second.autocorr) == 16 and second.autocorr.tobytes() == first.autocorr.tobytes()
    with np.load(os.path.join(dump_dir, "emi.npz")) as f:
        assert sorted(f.files) == ["autocorr", "temperature", "time series"]
        assert f["autocorr"].tobytes() == second.autocorr.tobytes()


@pytest.fixture(scope="module")
def two_way_pairs():
    """the pairs of a short two-way absorption run"""
    from renormalizer_amd.spectra import SpectraTwoWayPropZeroT

    class Keep(SpectraTwoWayPropZeroT):
        def process_mps(self, pair):
            self.__dict__.setdefault("pairs", []).append(pair)
            super().process_mps(pair)

    model = _holstein_test_model()
    job = Keep(model, "abs", OptimizeConfig(procedure=[[1, 0], [1, 0]]), offset=_offset(model),
               rng=np.random.default_rng(1))
    job.evolve(DT, 5)
    return job


def test_calc_ft_is_the_reference_expression(two_way_pairs):
    job = two_way_pairs
    assert len(job.pairs) == 6
    for pair, ft in zip(job.pairs, job.autocorr):
        bra, ket = pair
        ref = bra.conj().dot(ket) * np.conjugate(bra.coeff) * ket.coeff
        assert pair.ft == ft and pair.calc_ft() == ft
        assert abs(ft - ref) <= 1e-12 * abs(ref), (ft, ref)
    assert job.pairs[-1].ket_mps.is_complex and abs(job.autocorr[-1].imag) > 0


def test_overlap_leaves_its_operands_and_dot_alone(two_way_pairs):
    from renormalizer_amd.engine import get_engine
    bra, ket = two_way_pairs.pairs[-1]
    before = [t.to_host().copy() for t in list(bra) + list(ket)]
    handles = [t.ptr for t in list(bra) + list(ket)]
    d0 = bra.dot(ket, self_is_conj=False)
    s0 = get_engine().mps_overlap_stats()
    ov = bra.overlap(ket, self_is_conj=False)
    assert get_engine().mps_overlap_stats()["chain_kernel"] == s0["chain_kernel"] + 1
    d1 = bra.dot(ket, self_is_conj=False)
    assert (d0.real.hex(), d0.imag.hex()) == (d1.real.hex(), d1.imag.hex())
    assert abs(ov - d0) <= 1e-12 * abs(d0)
    assert handles == [t.ptr for t in list(bra) + list(ket)]
    for a, t in zip(before, list(bra) + list(ket)):
        assert np.array_equal(a, t.to_host())
