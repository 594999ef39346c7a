"""``SpinBosonDynamics`` (renormalizer_amd/sbm.py) on the GPU against the run of the reference in
tests/golden/tdvp_sbm_small.npz: a spin and five modes (omega = 0.5 .. 4, c = 0.3 / sqrt(1 .. 5), 5 levels), TDVP-PS
from the bond-expanded state the reference started from, dt = 0.1, five steps.  The job records the spin's density
matrix from ``Mps.site_rdms`` and the bond entropies from ``Mps.bond_entropies``."""
import os

import numpy as np
import pytest

from renormalizer_amd import (CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, Phonon, Quantity,
                              SpinBosonModel)

pytestmark = pytest.mark.gpu


def _model():
    omegas = np.linspace(0.5, 4.0, 5)
    cs = 0.3 / np.sqrt(np.arange(1, 6))
    ph_list = [Phonon.simple_phonon(Quantity(w), Quantity(c / w ** 2), 5) for w, c in zip(omegas, cs)]
    return SpinBosonModel(Quantity(0.0), Quantity(0.8), ph_list)


def _configs():
    return dict(compress_config=CompressConfig(CompressCriteria.fixed, max_bonddim=10),
                evolve_config=EvolveConfig(EvolveMethod.tdvp_ps))


@pytest.fixture(scope="module")
def run(golden_dir):
    from renormalizer_amd.mps.mps import Mps
    from renormalizer_amd.sbm import SpinBosonDynamics
    z = np.load(os.path.join(golden_dir, "tdvp_sbm_small.npz"))
    model = _model()
    n = int(z["init_nsite"])
    assert n == len(model.basis)
    for i, b in enumerate(model.basis):
        assert np.array_equal(np.asarray(b.sigmaqn).reshape(b.nbas, -1), z[f"sigmaqn_{i}"])

    class FromFixture(SpinBosonDynamics):
        def init_mps(self):
            mps = Mps.from_arrays(self.model, [z[f"init_site_{i}"] for i in range(n)],
                                  [z[f"init_qn_{i}"] for i in range(n + 1)], int(z["init_qnidx"]), z["init_qntot"],
                                  bool(z["init_to_right"]), complex(z["init_coeff"]))
            mps.compress_config = self.compress_config
            mps.evolve_config = self.evolve_config
            return mps

    job = FromFixture(model, **_configs())
    job.evolve(evolve_dt=float(z["dt"]), nsteps=5)
    return z, job


def test_series_against_the_reference(run):
    z, job = run
    assert float(z["dt"]) == 0.1 and len(job.evolve_times) == 6
    ref = z["obs_values"]
    dz, dx = np.abs(np.array(job.sigma_z) - ref[:, 0]).max(), np.abs(np.array(job.sigma_x) - ref[:, 1]).max()
    print(f"max |sigma_z - reference| = {dz:.2e}, max |sigma_x - reference| = {dx:.2e}")
    assert dz < 1e-8 and dx < 1e-8
    assert abs(job.sigma_z[0] - 1) < 1e-12 and job.sigma_z[-1] < 0.999          # the spin started up and moved
    for rho in job.rho:
        assert rho.shape == (2, 2)
        assert np.abs(rho - rho.conj().T).max() < 1e-10 and abs(np.trace(rho) - 1) < 1e-10


def test_bond_entropies_of_the_job(run):
    z, job = run
    n = len(job.latest_mps)
    assert len(job.bond_entropy) == 6 and all(np.shape(s) == (n - 1,) for s in job.bond_entropy)
    ref = job.latest_mps.calc_entropy("bond")
    print(f"max |bond_entropy - calc_entropy| = {np.abs(job.bond_entropy[-1] - ref).max():.2e}")
    assert np.abs(job.bond_entropy[-1] - ref).max() < 1e-10
    assert np.abs(job.bond_entropy[0]).max() < 1e-10 and job.bond_entropy[-1].max() > 1e-4    # entanglement grew


def test_dump_dict(run):
    d = run[1].get_dump_dict()
    assert list(d) == ["time series", "sigma_x", "sigma_z", "rho", "bond_entropy"]
    assert len(d["time series"]) == len(d["sigma_x"]) == len(d["sigma_z"]) == len(d["rho"]) == len(d["bond_entropy"]) == 6


def test_initial_state_of_the_job():
    """the reference's init_mps: the product state, padded with 1e-16 under TDVP when auto_expand is set"""
    from renormalizer_amd.sbm import SpinBosonDynamics, SpectralDensityFunction, param2mollist    # noqa: F401
    import renormalizer_amd
    assert renormalizer_amd.SpinBosonDynamics is SpinBosonDynamics
    model = _model()
    job = SpinBosonDynamics(model, **_configs())
    dims = list(job.latest_mps.bond_dims)
    assert dims[0] == dims[-1] == 1 and max(dims) > 1 and max(dims) <= 10
    assert len(job.sigma_z) == 1 and abs(job.sigma_z[0] - 1) < 1e-12 and abs(job.sigma_x[0]) < 1e-12
    assert np.abs(job.bond_entropy[0]).max() < 1e-10                # the padding carries weight 1e-32
    plain = SpinBosonDynamics(model, auto_expand=False, **_configs())
    assert all(d == 1 for d in plain.latest_mps.bond_dims)
    assert np.abs(plain.latest_mps.bond_entropies()).max() < 1e-12
    assert np.abs(plain.bond_entropy[0]).max() < 1e-12
