"""Base of the time-domain spectra jobs (renormalizer/spectra/base.py:11-46)."""
import numpy as np

from ..mps.mpo import Mpo
from ..utils import CompressConfig, Quantity
from ..utils.tdmps import TdMpsJob


class SpectraTdMpsJobBase(TdMpsJob):
    """model: the system; spectratype: "abs" (0-exciton initial state) or "emi" (1-exciton); temperature: a
    ``Quantity``; offset: energy subtracted from the Hamiltonian (``h_mpo = Mpo(model, offset=offset)``) so that the
    recorded function oscillates slowly.  ``process_mps`` records the overlap of every ``BraKetPair``."""

    def __init__(self, model, spectratype, temperature, evolve_config=None, compress_config=None, offset=Quantity(0),
                 dump_dir=None, job_name=None):
        self.model = model
        if spectratype not in ("emi", "abs"):
            raise ValueError(f"spectratype must be 'abs' or 'emi', got {spectratype!r}")
        self.spectratype = spectratype
        self.nexciton = 1 if spectratype == "emi" else 0
        self.compress_config = CompressConfig() if compress_config is None else compress_config
        self.temperature = temperature
        self.h_mpo = Mpo(model, offset=offset)
        self._autocorr = []
        super().__init__(evolve_config=evolve_config, dump_dir=dump_dir, job_name=job_name)

    def process_mps(self, braket_pair):
        self._autocorr.append(braket_pair.ft)

    @property
    def autocorr(self):
        return np.array(self._autocorr)

    def get_dump_dict(self):
        return {"temperature": self.temperature.as_au(), "time series": self.evolve_times, "autocorr": self.autocorr}
