"""``transport.SpectralFunctionZT`` on the GPU against the reference's own run (tests/golden/spectral_function_zt.npz,
written by tools/capture_spectral_function.py) and against dense propagation.

The model: a ``TI1DModel`` of 3 cells, each a simple electron and an oscillator with 3 levels (omega = 1), Holstein
coupling g = 0.7, hopping 0.5; TDVP-PS with a fixed bond limit of 64, 5 steps of 0.5.  At this size nothing is
truncated (the reference's ket bonds are 1, 2, 6, 9, 6, 3, 1) and the Hilbert space has 216 states, so
G_i(t) = -i <gs| a_i exp(-i (H - E0) t) a_0^+ |gs> is available from ``scipy.linalg.expm``.

Tolerance against the dense values and against the fixture: 1e-8 with max |G| = 1.  The reference itself is 2.0e-10 from
the dense values on exactly this input (the fixture records it); 1e-8 is the tighter end of what the README holds
observables to against the reference and 50 times the reference's own deviation, which leaves room for a different
Krylov stopping point.  Should the recorded path of before this job, ``evolve`` + ``expectations(a_opers, gs.conj())``,
exceed 1e-8 itself, that is a finding about ``evolve``: the new path is then held to that deviation plus 1e-10.
Measured on the MI355X: see profiles/trdm1.md."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OMEGA, G, HOP, NCELL, NLEVEL, NSTEPS, TIME = 1.0, 0.7, 0.5, 3, 3, 5, 2.5
TOL = 1e-8


def _model():
    from renormalizer_amd.model.basis import BasisSHO, BasisSimpleElectron
    from renormalizer_amd.model.model import TI1DModel
    from renormalizer_amd.model.op import Op
    basis = [BasisSimpleElectron("e"), BasisSHO("ph", OMEGA, NLEVEL)]
    local = [Op(r"a^\dagger a", "e", G ** 2 * OMEGA), Op(r"b^\dagger b", "ph", OMEGA),
             -G * OMEGA * Op(r"a^\dagger a", "e") * Op(r"b^\dagger + b", "ph")]
    hopping = [Op(r"a^\dagger a", [(0, "e"), (1, "e")], HOP), Op(r"a^\dagger a", [(1, "e"), (0, "e")], HOP)]
    return TI1DModel(basis, local, hopping, NCELL)


@pytest.fixture(scope="module")
def run():
    """(job, trdm1 stats before, after, G of the path of before this job per recorded step, gs, the first ket)"""
    from renormalizer_amd.engine import get_engine
    from renormalizer_amd.mps.mpo import Mpo
    from renormalizer_amd.transport import SpectralFunctionZT
    from renormalizer_amd.utils import CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod

    class Recording(SpectralFunctionZT):
        def process_mps(self, mps):
            super().process_mps(mps)
            gs, ket = mps
            a_opers = [Mpo.onsite(self.model, "a", dof_set={dof}) for dof in self.model.e_dofs]
            self.__dict__.setdefault("old_G", []).append(np.asarray(ket.expectations(a_opers, gs.conj())) / 1j)

    eng = get_engine()
    s0 = eng.mps_trdm1_stats()
    job = Recording(_model(), CompressConfig(CompressCriteria.fixed, max_bonddim=64), EvolveConfig(EvolveMethod.tdvp_ps))
    job.evolve(nsteps=NSTEPS, evolve_time=TIME)
    return job, s0, eng.mps_trdm1_stats(), np.array(job.old_G)


@pytest.fixture(scope="module")
def dense(run):
    """G by dense propagation, shape (NSTEPS + 1, 3)"""
    import scipy.linalg
    from renormalizer_amd.mps.mpo import Mpo
    job = run[0]
    model = job.model
    gs = np.asarray(job.latest_mps[0].todense()).reshape(-1)
    h = np.asarray(Mpo(model).todense())
    assert h.shape == (216, 216) and abs(np.linalg.norm(gs) - 1) < 1e-14
    e0 = (gs.conj() @ h @ gs).real
    a = [np.asarray(Mpo.onsite(model, "a", dof_set={dof}).todense()) for dof in model.e_dofs]
    ket0 = a[0].conj().T @ gs
    u = scipy.linalg.expm(-1j * (h - e0 * np.eye(216)) * (TIME / NSTEPS))
    rows, ket = [], ket0
    for _ in range(NSTEPS + 1):
        rows.append([-1j * (gs.conj() @ ai @ ket) for ai in a])
        ket = u @ ket
    return np.array(rows)


def test_green_function(run, dense, golden_dir):
    job, _, _, old_g = run
    z = np.load(os.path.join(golden_dir, "spectral_function_zt.npz"))
    g = job.G_array
    assert g.shape == (NSTEPS + 1, NCELL) and g.dtype == np.complex128
    assert np.allclose(job.evolve_times, z["time series"], rtol=0, atol=1e-14)
    assert list(job.latest_mps[1].bond_dims) == list(z["ket bond dims"]) == [1, 2, 6, 9, 6, 3, 1]
    dev_new, dev_old = np.abs(g - dense).max(), np.abs(old_g - dense).max()
    dev_fix, dev_ref = np.abs(g - z["G array"]).max(), float(z["reference deviation from dense"])
    print(f"max |G - dense|: one-call path {dev_new:.2e}, evolve + expectations {dev_old:.2e}, the reference "
          f"{dev_ref:.2e}; max |G - reference| = {dev_fix:.2e}; max |G| = {np.abs(dense).max():.3f}")
    bound = TOL if dev_old <= TOL else dev_old + 1e-10
    assert dev_new <= bound and dev_fix <= bound
    assert np.abs(g - old_g).max() <= 1e-10                              # the same states, two ways to the numbers
    # G(0) = -i delta_i0.  Exact for a_0^+ |gs>; the ket of a TDVP run is that state plus the admixture of
    # expand_bond_dimension (coef = 1e-10 of a state of comparable norm), so the row is held to the bound of all rows
    assert abs(g[0, 0] + 1j) < 1e-12 and np.abs(g[0] - np.array([-1j, 0, 0])).max() <= bound
    assert np.abs(g[:, 1] - g[:, 2]).max() <= bound                      # a ring of three: |i - j| = 1 and 2 agree
    assert np.abs(g[1:, 1]).min() > 1e-2                                 # and are no zeros
    occ = np.array(job.e_occupations_array)
    dev_occ = np.abs(occ - z["electron occupations array"]).max()
    print(f"max |occupations - reference| = {dev_occ:.2e}")
    assert occ.shape == (NSTEPS + 1, NCELL) and dev_occ <= bound and np.abs(occ.sum(axis=1) - 1).max() < 1e-9


def test_one_engine_call_per_recorded_step(run):
    _, s0, s1, _ = run
    calls = s1["chain_kernel"] + s1["enqueued"] - s0["chain_kernel"] - s0["enqueued"]
    assert calls == NSTEPS + 1 and s1["matrices"] - s0["matrices"] == (NSTEPS + 1) * NCELL
    assert s1["sites"] - s0["sites"] == (NSTEPS + 1) * 2 * NCELL


def test_dump(run, golden_dir):
    job = run[0]
    z = np.load(os.path.join(golden_dir, "spectral_function_zt.npz"))
    dump = job.get_dump_dict()
    assert list(dump) == ["temperature", "time series", "G array", "Gk array", "electron occupations array"]
    assert dump["temperature"] == 0 and np.array_equal(dump["G array"], job.G_array)
    assert dump["Gk array"].shape == (NSTEPS + 1, NCELL // 2 + 1)
    assert np.abs(dump["Gk array"] - z["Gk array"]).max() <= NCELL * TOL
