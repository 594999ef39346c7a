"""Charge diffusion in a Holstein chain (renormalizer/transport/dynamics.py): an electron is created on the centre
molecule, on top of the phonon vacuum (``InitElectron.fc``), of phonons already relaxed around the charge
(``InitElectron.relaxed``) or of the purified thermal phonon state (``temperature`` > 0), and the state is propagated in
real time.  After every step the job records the energy, the occupations, the mean square displacement and the bond
entropies; with ``rdm=True`` also the reduced density matrix of the electron rho_ij = <a_i^+ a_j>, which comes from
``Mps.edof_rdm()``: one walk over the chain inside the engine (``mpse_mps_corr``).  The k-space occupations, the
electron-phonon entropy and the coherence length are host arithmetic on rho."""
import logging
import os
from collections import OrderedDict
from enum import Enum

import numpy as np

from ..mps.mpdm import MpDm
from ..mps.mpo import Mpo
from ..mps.mps import Mps
from ..utils import CompressConfig, Quantity
from ..utils.tdmps import TdMpsJob

logger = logging.getLogger("renormalizer_amd")

EDGE_THRESHOLD = 1e-4


class InitElectron(Enum):
    """How the initial state of the charge is prepared"""
    fc = "franck-condon excitation"
    relaxed = "analytically relaxed phonon(s)"


def calc_r_square(e_occupations):
    """<r^2> - <r>^2 of a distribution over the sites 0, 1, ..; 0 for an empty chain (dynamics.py:289-295)"""
    occ = np.asarray(e_occupations, dtype=float)
    if np.allclose(occ, 0.0):
        return 0
    r = np.arange(len(occ), dtype=float)
    total = occ.sum()
    mean_r = (r * occ).sum() / total
    return float((r * r * occ).sum() / total - mean_r ** 2)


def k_occupations(rdm):
    """Occupations of |k> = sum_j exp(-i j k) |j> / sqrt(N), k from -pi in steps of 2 pi / N (dynamics.py:212-217)"""
    rdm = np.asarray(rdm)
    n = rdm.shape[0]
    k = (np.arange(-n, n, 2) / n * np.pi).reshape(-1, 1)
    transform = np.exp(-1j * k * np.arange(0, n).reshape(1, -1)) / np.sqrt(n)
    return np.diag(transform @ rdm @ transform.conj().T).real


def eph_vn_entropy(rdm):
    """-Tr rho ln rho of the electron's density matrix, from its eigenvalues (the reference takes a matrix logarithm,
    dynamics.py:220)"""
    rdm = np.asarray(rdm)
    w = np.linalg.eigvalsh((rdm + rdm.conj().T) / 2)
    w = w[w > 0]
    return float(-(w * np.log(w)).sum())


def coherent_length(rdm):
    """L = sum_{i != j} |rho_ij| (dynamics.py:223)"""
    rdm = np.asarray(rdm)
    return float(np.abs(rdm).sum() - np.trace(rdm).real)


class ChargeDiffusionDynamics(TdMpsJob):
    """model: a ``HolsteinModel``; temperature: ``Quantity``, zero for a pure state; compress_config / evolve_config: of
    the state; stop_at_edge: end the run when the occupation of the first molecule exceeds ``EDGE_THRESHOLD``;
    init_electron: an ``InitElectron``; rdm: record the reduced density matrix of the electron and what follows from it;
    dump_dir / job_name: where the results go, and ``<dump_dir>/<job_name>_impdm.npz`` is where the thermal state is
    read from when the file exists and written to when it does not.

    Recorded per step: ``energies``, ``r_square_array``, ``e_occupations_array``, ``ph_occupations_array``,
    ``bond_vn_entropy_array``, and with ``rdm=True`` ``reduced_density_matrices``, ``k_occupations_array``,
    ``eph_vn_entropy_array``, ``coherent_length_array``."""

    def __init__(self, model, temperature: Quantity = Quantity(0, "K"), compress_config: CompressConfig = None,
                 evolve_config=None, stop_at_edge: bool = True, init_electron=InitElectron.relaxed, rdm: bool = False,
                 dump_dir: str = None, job_name: str = None):
        self.model = model
        self.temperature = temperature
        self.mpo = None
        self.init_electron = init_electron
        self.compress_config = CompressConfig() if compress_config is None else compress_config
        self.energies = []
        self.r_square_array = []
        self.e_occupations_array = []
        self.ph_occupations_array = []
        self.reduced_density_matrices = [] if rdm else None
        self.k_occupations_array = []
        self.eph_vn_entropy_array = []     # von Neumann entropy between the electron and the phonons
        self.bond_vn_entropy_array = []    # entropy at each bond
        self.coherent_length_array = []
        if dump_dir is not None and job_name is not None:
            self.thermal_dump_path = os.path.join(dump_dir, job_name + "_impdm.npz")
        else:
            self.thermal_dump_path = None
        self.thermal_state_loaded = False
        self.stop_at_edge = stop_at_edge
        self.custom_dump_info = OrderedDict()
        super().__init__(evolve_config=evolve_config, dump_dir=dump_dir, job_name=job_name)
        assert self.mpo is not None

    @property
    def mol_num(self):
        return self.model.mol_num

    # ------------------------------------------------------------------ initial state
    def _thermal_state(self):
        """The purified thermal state of the phonons without the electron, rho(beta / 2): exact, because the
        electron-free Hamiltonian is a sum of one-site terms (``Mpo.exact_propagator``, space "GS"); in max(20, N)
        steps with a normalisation after each, so that no factor leaves the range of a double.  With a dump path every
        job starts from the file's state, the one that wrote it included."""
        path = self.thermal_dump_path
        if path is not None and os.path.exists(path):
            self.thermal_state_loaded = True
            logger.info(f"thermal state read from {path}")
            return MpDm.load(self.model, path)
        mpdm = MpDm.max_entangled_gs(self.model)
        h_mpo = Mpo(self.model)
        nsteps = max(20, len(mpdm))
        dtau = self.temperature.to_beta() / 2 / nsteps
        for _ in range(nsteps):
            energy = np.real(mpdm.expectation(h_mpo))
            mpdm = Mpo.exact_propagator(self.model, -dtau, space="GS", shift=-energy).apply(mpdm, canonicalise=True)
            mpdm.normalize("mps_and_coeff")
        if path is None:
            return mpdm
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        mpdm.dump(path)
        return MpDm.load(self.model, path)

    def _creation_operator(self):
        return Mpo.onsite(self.model, r"a^\dagger", dof_set={self.mol_num // 2})

    def create_electron_fc(self, gs_mp):
        return self._creation_operator().apply(gs_mp)

    def create_electron_relaxed(self, gs_mp):
        """the phonons of the centre molecule start in the eigenbasis of the displaced oscillator
        (``Phonon.get_displacement_evecs``): for a pure state, its ground state"""
        assert np.allclose(gs_mp.bond_dims, np.ones_like(gs_mp.bond_dims))
        centre = self.mol_num // 2
        for i, ph in enumerate(self.model[centre].ph_list):
            idx = self.model.dof_to_siteidx[(centre, i)]
            mt = gs_mp[idx].to_host()[0, ..., 0]
            mt = ph.get_displacement_evecs().dot(mt)
            gs_mp[idx] = mt.reshape([1] + list(mt.shape) + [1])
        return self._creation_operator().apply(gs_mp)

    def create_electron(self, gs_mp):
        logger.info(f"Creating electron using {self.init_electron}")
        method = {InitElectron.fc: self.create_electron_fc, InitElectron.relaxed: self.create_electron_relaxed}
        return method[self.init_electron](gs_mp)

    def init_mps(self):
        tentative_mpo = Mpo(self.model)
        if self.temperature == 0:
            gs_mp = Mps.ground_state(self.model, max_entangled=False)
        else:
            gs_mp = self._thermal_state()
        init_mp = self.create_electron(gs_mp)
        energy = Quantity(np.real(init_mp.expectation(tentative_mpo)))
        self.mpo = Mpo(self.model, offset=energy)
        logger.info(f"mpo bond dims: {self.mpo.bond_dims}")
        init_mp.evolve_config = self.evolve_config
        init_mp.compress_config = self.compress_config
        if self.evolve_config.is_tdvp:
            init_mp = init_mp.expand_bond_dimension(self.mpo)
        init_mp.canonicalise()
        return init_mp

    # ------------------------------------------------------------------ per step
    def process_mps(self, mps):
        new_energy = mps.expectation(self.mpo)
        self.energies.append(new_energy)
        logger.debug(f"Energy: {new_energy}")
        if self.reduced_density_matrices is not None:
            rdm = mps.edof_rdm()
            self.reduced_density_matrices.append(rdm)
            assert rdm.shape == (self.mol_num, self.mol_num)
            self.k_occupations_array.append(k_occupations(rdm))
            self.eph_vn_entropy_array.append(eph_vn_entropy(rdm))
            self.coherent_length_array.append(coherent_length(rdm))
            e_occupations = np.diag(rdm).real
        else:
            e_occupations = np.real(mps.e_occupations)
        self.e_occupations_array.append(e_occupations)
        self.r_square_array.append(calc_r_square(e_occupations))
        self.ph_occupations_array.append(np.real(mps.ph_occupations))
        logger.info(f"e occupations: {self.e_occupations_array[-1]}")
        bond_vn_entropy = mps.calc_bond_entropy()
        logger.info(f"bond entropy: {bond_vn_entropy}")
        self.bond_vn_entropy_array.append(bond_vn_entropy)

    def evolve_single_step(self, evolve_dt):
        return self.latest_mps.evolve(self.mpo, evolve_dt)

    def stop_evolve_criteria(self):
        """the electron has reached the edge"""
        return bool(self.stop_at_edge and EDGE_THRESHOLD < self.e_occupations_array[-1][0])

    # ------------------------------------------------------------------ results
    def get_dump_dict(self):
        dump_dict = OrderedDict()
        dump_dict["mol list"] = self.model.to_dict()
        dump_dict["tempearture"] = self.temperature.as_au()            # (sic: the reference's key)
        dump_dict["total time"] = self.evolve_times[-1]
        dump_dict["other info"] = self.custom_dump_info
        dump_dict["r square array"] = self.r_square_array
        dump_dict["electron occupations array"] = self.e_occupations_array
        dump_dict["phonon occupations array"] = self.ph_occupations_array
        dump_dict["k occupations array"] = self.k_occupations_array
        dump_dict["eph entropy"] = self.eph_vn_entropy_array
        dump_dict["bond entropy"] = self.bond_vn_entropy_array
        dump_dict["coherent length array"] = self.coherent_length_array
        if self.reduced_density_matrices:
            dump_dict["reduced density matrices"] = self.reduced_density_matrices
        dump_dict["time series"] = list(self.evolve_times)
        return dump_dict

    def is_similar(self, other: "ChargeDiffusionDynamics", rtol=1e-3):
        """the same number of steps and every recorded series equal to ``rtol`` (and 1e-3 absolute)"""
        if len(self.evolve_times) != len(other.evolve_times):
            return False
        series = ("evolve_times", "r_square_array", "energies", "e_occupations_array", "ph_occupations_array",
                  "coherent_length_array")
        return all(np.allclose(getattr(self, name), getattr(other, name), rtol=rtol, atol=1e-3) for name in series)
