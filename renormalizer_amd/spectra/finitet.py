"""Finite-temperature absorption / emission in the time domain by purification
(renormalizer/spectra/finitet.py:16-150): bra and ket are density operators in MPS form (``MpDm``),
C(t) = Tr[(mu rho^1/2)^+(t) (mu rho^1/2)(t)]."""
import logging
import os

import numpy as np

from ..mps.mpdm import MpDm
from ..mps.mpo import Mpo
from ..mps.mps import BraKetPair
from ..utils import CompressConfig, EvolveConfig
from .base import SpectraTdMpsJobBase

logger = logging.getLogger("renormalizer_amd")


class BraKetPairEmiFiniteT(BraKetPair):
    def calc_ft(self):
        return np.conj(super().calc_ft())


class BraKetPairAbsFiniteT(BraKetPair):
    pass


class SpectraFiniteT(SpectraTdMpsJobBase):
    """temperature: a ``Quantity``; insteps: imaginary-time steps of the thermal state (emission; absorption starts in
    the exciton-free space, where the thermal state is propagated exactly); icompress_config / ievolve_config: of the
    imaginary-time propagation.  With ``dump_dir`` and ``job_name`` the thermal state of an emission job is written to
    ``<dump_dir>/<job_name>_impo.npz`` and read back by the next job of that name instead of being propagated again."""

    def __init__(self, model, spectratype, temperature, insteps, offset, evolve_config=None, icompress_config=None,
                 ievolve_config=None, dump_dir=None, job_name=None):
        self.insteps = insteps
        self.icompress_config = CompressConfig() if icompress_config is None else icompress_config
        self.ievolve_config = EvolveConfig() if ievolve_config is None else ievolve_config
        self.thermal_state_loaded = False
        # TdMpsJob.__init__ calls init_mps, which needs these before the base classes have run
        self.temperature, self.dump_dir, self.job_name = temperature, dump_dir, job_name
        super().__init__(model, spectratype, temperature, evolve_config=evolve_config, offset=offset, dump_dir=dump_dir,
                         job_name=job_name)

    def init_mps(self):
        return self.init_mps_emi() if self.spectratype == "emi" else self.init_mps_abs()

    @property
    def _thermal_dump_path(self):
        assert self._defined_output_path
        return os.path.join(self.dump_dir, self.job_name + "_impo.npz")

    def _thermal_state_emi(self):
        """rho(beta / 2) of the one-exciton space.  With an output path every job starts from the file's state, the
        one that wrote it included: a repeated job then reproduces the series bit for bit."""
        from ..mps.thermalprop import thermal_state
        if self._defined_output_path and os.path.exists(self._thermal_dump_path):
            self.thermal_state_loaded = True
            logger.info(f"thermal state read from {self._thermal_dump_path}")
            return MpDm.load(self.model, self._thermal_dump_path)
        i_mpo = MpDm.max_entangled_ex(self.model)
        i_mpo.compress_config = self.icompress_config
        i_mpo.evolve_config = self.ievolve_config
        beta = self.temperature.to_beta()
        ket_mpo, _ = thermal_state(i_mpo, Mpo(self.model), beta / 2j / self.insteps, self.insteps)
        if not self._defined_output_path:
            return ket_mpo
        os.makedirs(self.dump_dir, exist_ok=True)
        ket_mpo.dump(self._thermal_dump_path)
        return MpDm.load(self.model, self._thermal_dump_path)

    def init_mps_emi(self):
        ket_mpo = self._thermal_state_emi()
        ket_mpo.evolve_config = self.evolve_config
        # rho^1/2 a^+: the operator acts on the lower legs (finitet.py:96-100)
        dipole_dagger = Mpo.onsite(self.model, "a", dipole=True).conj_trans()
        a_ket_mpo = ket_mpo.apply(dipole_dagger, canonicalise=True)
        if self.evolve_config.is_tdvp:
            a_ket_mpo = a_ket_mpo.expand_bond_dimension(self.h_mpo)
        a_ket_mpo.normalize("mps_norm_to_coeff")
        return BraKetPairEmiFiniteT(a_ket_mpo.copy(), a_ket_mpo)

    def init_mps_abs(self):
        dipole_mpo = Mpo.onsite(self.model, r"a^\dagger", dipole=True)
        beta = self.temperature.to_beta()
        # no exciton: the Hamiltonian is the sum of the local vibrational ones, propagated exactly and normalised
        ket_mpo = MpDm.max_entangled_gs(self.model).evolve_exact(Mpo(self.model), beta / 2j, "GS")
        ket_mpo.normalize("mps_and_coeff")
        ket_mpo.compress_config = self.icompress_config
        ket_mpo.evolve_config = self.evolve_config
        a_ket_mpo = dipole_mpo.apply(ket_mpo, canonicalise=True)
        if self.evolve_config.is_tdvp:
            a_ket_mpo = a_ket_mpo.expand_bond_dimension(self.h_mpo)
        a_ket_mpo.normalize("mps_norm_to_coeff")
        return BraKetPairAbsFiniteT(a_ket_mpo.copy(), a_ket_mpo)

    def evolve_single_step(self, evolve_dt):
        bra, ket = self.latest_mps
        if len(self.evolve_times) % 2 == 1:
            ket = ket.evolve_exact(self.h_mpo, -evolve_dt, "GS").evolve(self.h_mpo, evolve_dt)
        else:
            bra = bra.evolve_exact(self.h_mpo, evolve_dt, "GS").evolve(self.h_mpo, -evolve_dt)
        return self.latest_mps.__class__(bra, ket)

    def stop_evolve_criteria(self):
        """the last ten values have died out: |mean| and spread below 1e-5 of C(0) (finitet.py:116-122)"""
        corr = self.autocorr
        if len(corr) < 10:
            return False
        last, first = corr[-10:], corr[0]
        return bool(np.abs(last.mean()) < 1e-5 * np.abs(first) and last.std() < 1e-5 * np.abs(first))
