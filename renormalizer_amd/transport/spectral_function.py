"""One-particle retarded Green's function at zero temperature of a translationally invariant one-dimensional model
(renormalizer/transport/spectral_function.py):

    i G_ij(t) = <0| c_i(t) c_j^+ |0>

With translational invariance G depends on |i - j| alone, so the electron is created on the first electronic degree of
freedom, ket = a_0^+ |gs>, only the ket is propagated (with the Hamiltonian shifted by the energy of |gs>), and after
every step the job records G_i(t) = <gs| a_i |ket(t)> / 1j for every electronic degree of freedom i.  That row is
``gs.transition_elements("a", model.e_dofs, ket, self_is_conj=False)``: one walk over the two chains inside the engine
(``mpse_mps_trdm1``) instead of one operator window, one closing product and one host read per degree of freedom and a
conjugated copy of the bra per step.  In k space

    G_k(t) = sum_d G_d(t) exp(i k d),   k = 0, 2 pi / N, .., pi

is what ``get_dump_dict`` stores as ``"Gk array"``; the spectral function A(k, omega) = -1 / pi Im int_0^inf dt exp(i
omega t) G_k(t) is left to the user, as in the reference, since it wants a broadening and a frequency window chosen with
knowledge of the model.  For a finite temperature the reference recommends thermofield dynamics with a transformed
Hamiltonian (J. Chem. Phys. 145, 224101 (2016)); bra and ket then both have bonds above 1, which the engine call takes
as well."""
import logging

import numpy as np

from ..mps.mpo import Mpo
from ..mps.mps import Mps
from ..utils import CompressConfig, Quantity
from ..utils.tdmps import TdMpsJob

logger = logging.getLogger("renormalizer_amd")


class SpectralFunctionZT(TdMpsJob):
    """model: a ``TI1DModel`` (a custom ``Model`` works when the user sees to the translational invariance; an even
    number of electronic degrees of freedom makes k = pi well defined); compress_config / evolve_config: of the ket;
    dump_dir / job_name: where the results go.

    Recorded per step: ``G_array`` (time, |i - j|) and ``e_occupations_array``."""

    def __init__(self, model, compress_config: CompressConfig = None, evolve_config=None, dump_dir: str = None,
                 job_name: str = None):
        self.model = model
        self.compress_config = CompressConfig() if compress_config is None else compress_config
        self._G_array = []                  # electron-addition Green's function at every recorded time
        self.e_occupations_array = []
        self.temperature = Quantity(0)
        super().__init__(evolve_config=evolve_config, dump_dir=dump_dir, job_name=job_name)

    @property
    def G_array(self):
        """G_ij(t) as a two-dimensional array: first index t, second index |i - j|"""
        return np.array(self._G_array)

    def init_mps(self):
        creation_oper = Mpo.onsite(self.model, r"a^\dagger", dof_set={self.model.e_dofs[0]})
        gs = Mps.ground_state(self.model, False)
        self.h_mpo = Mpo(self.model, offset=Quantity(gs.expectation(Mpo(self.model))))
        a_ket = creation_oper.apply(gs, canonicalise=True)
        a_ket.compress_config = self.compress_config
        a_ket.evolve_config = self.evolve_config
        a_ket.normalize("mps_norm_to_coeff")
        if self.evolve_config.is_tdvp:
            a_ket = a_ket.expand_bond_dimension(self.h_mpo)
        return (gs, a_ket)

    def process_mps(self, mps):
        gs, a_ket = mps
        # <gs| a_i |ket> for every i from one engine call; gs is not conjugated beforehand
        self._G_array.append(gs.transition_elements("a", self.model.e_dofs, a_ket, self_is_conj=False) / 1j)
        self.e_occupations_array.append(a_ket.occupations()[0])

    def evolve_single_step(self, evolve_dt):
        gs, prev_ket = self.latest_mps
        return (gs, prev_ket.evolve(self.h_mpo, evolve_dt))

    def get_dump_dict(self):
        dump_dict = dict()
        dump_dict["temperature"] = self.temperature.as_au()
        dump_dict["time series"] = self.evolve_times
        dump_dict["G array"] = self.G_array
        ne = self.model.n_edofs
        kpoints_distance = (2 * np.pi) / ne
        n_kpoints = ne // 2 + 1
        ka = (np.arange(n_kpoints) * kpoints_distance).reshape(1, 1, -1)
        ijdiff = np.arange(ne).reshape(1, -1, 1)
        # Green's function in k space
        dump_dict["Gk array"] = np.sum(self.G_array.reshape(-1, ne, 1) * np.exp(1j * ka * ijdiff), axis=1)
        dump_dict["electron occupations array"] = self.e_occupations_array
        return dump_dict
