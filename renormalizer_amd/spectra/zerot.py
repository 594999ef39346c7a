"""Zero-temperature absorption / emission in the time domain (renormalizer/spectra/zerot.py:15-82)."""
from ..mps.mpo import Mpo
from ..mps.mps import BraKetPair, Mps
from ..utils import OptimizeConfig, Quantity
from .base import SpectraTdMpsJobBase


def dipole_on_ground_state(job, rng=None):
    """mu |psi0>, canonical, its norm moved to ``coeff``: psi0 from ``optimize_mps`` in the job's exciton sector under
    ``job.optimize_config`` (zerot.py:46-65)."""
    from ..mps.gs import optimize_mps
    i_mps = Mps.random(job.model, job.nexciton, job.optimize_config.procedure[0][0], 1, rng=rng)
    i_mps.optimize_config = job.optimize_config
    _, i_mps = optimize_mps(i_mps, job.h_mpo)
    operator = "a" if job.spectratype == "emi" else r"a^\dagger"
    a_ket_mps = Mpo.onsite(job.model, operator, dipole=True).apply(i_mps, canonicalise=True)
    return a_ket_mps


class SpectraZeroT(SpectraTdMpsJobBase):
    """model, spectratype ("abs" / "emi"); optimize_config: the ground-state sweep; evolve_config: the propagation;
    rng: generator of the random start state of the ground-state sweep."""

    def __init__(self, model, spectratype, optimize_config=None, evolve_config=None, compress_config=None,
                 offset=Quantity(0), dump_dir=None, job_name=None, rng=None):
        self.optimize_config = OptimizeConfig() if optimize_config is None else optimize_config
        self.rng = rng
        super().__init__(model, spectratype, Quantity(0), evolve_config, compress_config, offset, dump_dir, job_name)

    def init_mps(self):
        a_ket_mps = dipole_on_ground_state(self, self.rng)
        a_ket_mps.evolve_config = self.evolve_config
        a_ket_mps.compress_config = self.compress_config
        if self.evolve_config.is_tdvp:
            a_ket_mps = a_ket_mps.expand_bond_dimension(self.h_mpo)
        a_ket_mps.normalize("mps_norm_to_coeff")
        return BraKetPair(a_ket_mps.copy(), a_ket_mps)


class SpectraOneWayPropZeroT(SpectraZeroT):
    """the bra stays, the ket moves by dt"""

    def evolve_single_step(self, evolve_dt):
        bra, ket = self.latest_mps
        return BraKetPair(bra, ket.evolve(self.h_mpo, evolve_dt))


class SpectraTwoWayPropZeroT(SpectraZeroT):
    """bra and ket move alternately, the bra by -dt, the ket by +dt: half the time per state for the same C(t)"""

    def evolve_single_step(self, evolve_dt):
        bra, ket = self.latest_mps
        if len(self.evolve_times) % 2 == 1:
            ket = ket.evolve(self.h_mpo, evolve_dt)
        else:
            bra = bra.evolve(self.h_mpo, -evolve_dt)
        return BraKetPair(bra, ket)
