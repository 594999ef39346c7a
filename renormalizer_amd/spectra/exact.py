"""Zero-temperature spectra by the exact local propagator (renormalizer/spectra/exact.py:15-104): after the dipole
has acted the state lives in a space where the Hamiltonian is a sum of local vibrational ones ("GS" for emission of any
system, "EX" for absorption of a single molecule), so every step is one application of a bond-dimension-1 MPO.  The
bra's phase exp(i E t) is left out to keep the recorded function smooth."""
from ..mps.mps import BraKetPair
from ..utils import OptimizeConfig, Quantity
from .base import SpectraTdMpsJobBase
from .zerot import dipole_on_ground_state


class SpectraExact(SpectraTdMpsJobBase):
    def __init__(self, model, spectratype, optimize_config=None, offset=Quantity(0), dump_dir=None, job_name=None,
                 rng=None):
        if spectratype == "abs" and len(model.mol_list) != 1:
            raise ValueError("exact absorption needs a single molecule: the excited-state space is local only then")
        self.space = "GS" if spectratype == "emi" else "EX"
        self.optimize_config = OptimizeConfig() if optimize_config is None else optimize_config
        self.rng = rng
        super().__init__(model, spectratype, Quantity(0), offset=offset, dump_dir=dump_dir, job_name=job_name)

    def init_mps(self):
        a_ket_mps = dipole_on_ground_state(self, self.rng)
        a_ket_mps.normalize("mps_norm_to_coeff")
        return BraKetPair(a_ket_mps.copy(), a_ket_mps)

    def evolve_single_step(self, evolve_dt):
        bra, ket = self.latest_mps
        return BraKetPair(bra, ket.evolve_exact(self.h_mpo, evolve_dt, self.space))
