"""Correction-vector base class and frequency batches (renormalizer/cv/spectra_cv.py:16-204)."""
import logging

import numpy as np

from ..mps.mpo import Mpo
from ..utils import CompressConfig, CompressCriteria

logger = logging.getLogger("renormalizer_amd")


def batch_run(freq_reg, cores, obj, filename=None):
    """Spectrum over the frequencies ``freq_reg`` with one ``SpectraCv`` object (spectra_cv.py:17-49).  The reference
    hands the frequencies to a pool of ``cores`` processes; its pool is a CPU device, here every process would open the
    GPU, so the frequencies run one after another in this process whatever ``cores`` says.  ``filename``: the results so
    far are saved (``np.save``) after every frequency.  Returns the list of spectral values."""
    logger.info(f"{len(freq_reg)} total frequency points to do")
    assert cores >= 1
    if cores > 1:
        logger.info(f"cores = {cores}: no process pool on the GPU engine, the frequencies run one after another in "
                    f"this process")
    spectra = []
    obj.batch_run = True
    for omega in freq_reg:
        spectra.append(obj.cv_solve(omega))
        if filename is not None:
            np.save(f"{filename}", spectra)
    return spectra


class SpectraCv:
    """The sweep loop of the correction-vector method (spectra_cv.py:52-204); the subclass supplies the right-hand
    side, the start vector, the operator and the centre solve."""

    def __init__(self, model, spectratype, m_max, eta, h_mpo=None, method="1site", procedure_cv=None, rtol=1e-5,
                 b_mps=None, e0=None, cv_mps=None):
        self.model = model
        assert spectratype in ["abs", "emi", None]
        self.spectratype = spectratype
        self.m_max = m_max
        self.eta = eta
        self.h_mpo = Mpo(model) if h_mpo is None else h_mpo
        assert method in ["1site", "2site"]
        self.method = method
        logger.info(f"cv optimize method: {method}")
        # percent of the slots shared equally between the quantum-number blocks in each sweep (select_basis)
        if procedure_cv is None:
            procedure_cv = [0.4, 0.4, 0.2, 0.2, 0.1, 0.1] + [0] * 45
        self.procedure_cv = procedure_cv
        self.rtol = rtol
        # A x = b: the right-hand side and, at zero temperature, the ground-state energy
        if b_mps is None:
            self.b_mps, self.e0 = self.init_b_mps()
        else:
            self.b_mps = b_mps
            self.e0 = e0
        self.cv_mps = self.init_cv_mps() if cv_mps is None else cv_mps
        self.cv_mps.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=m_max)
        self.hop_time = []
        self.macro_iteration_result = []
        self.batch_run = False
        logger.info("DDMRG job created.")

    def cv_solve(self, omega):
        """The spectral value at ``omega``: sweeps over the correction vector until the two largest sweep results
        agree to ``rtol`` (spectra_cv.py:119-176)."""
        converged = False
        len_cv = len(self.cv_mps)
        self.oper_prepare(omega)
        lr_group = None
        isweep = 0
        for idx, procedure in enumerate(self.procedure_cv):
            isweep = idx + 1
            first = 1 if self.method == "1site" else 2
            if self.cv_mps.to_right and self.cv_mps.qnidx == 0:
                irange = np.arange(first, len_cv + 1)
            elif (not self.cv_mps.to_right) and self.cv_mps.qnidx == self.cv_mps.site_num - 1:
                irange = np.arange(len_cv, first - 1, -1)
            else:
                assert False
            if isweep == 1:
                lr_group = self.initialize_LR()
            micro_iteration_result = []
            for isite in irange:
                l_value = self.optimize_cv(lr_group, isite, percent=procedure)
                at_end = (not self.cv_mps.to_right and isite == 1) or (self.cv_mps.to_right and isite == len_cv)
                if not (self.method == "1site" and at_end):
                    lr_group = self.update_LR(lr_group, isite)
                micro_iteration_result.append(-1.0 / (np.pi * self.eta) * l_value)
                logger.debug(f"omega:{omega}, isweep:{isweep}, isite:{isite}, bond dims:{self.cv_mps.bond_dims}, "
                             f"response result:{micro_iteration_result[-1]}")
            self.cv_mps.to_right = not self.cv_mps.to_right
            self.macro_iteration_result.append(max(micro_iteration_result))
            if idx > 0 and procedure == 0:
                v1, v2 = sorted(self.macro_iteration_result)[-2:]
                if abs((v1 - v2) / v1) < self.rtol:
                    converged = True
                    break
        if converged:
            logger.info("cv converged!")
        else:
            logger.warning("cv *NOT* converged!")
        res = max(self.macro_iteration_result)
        logger.info(f"omega:{omega}, sweeps:{isweep}, average_hop:{int(np.mean(self.hop_time))},res:{res}")
        if self.batch_run:
            self.clear_res()      # the object goes on to the next frequency
        return res

    def clear_res(self):
        self.hop_time.clear()
        self.macro_iteration_result.clear()

    def init_cv_mps(self):
        raise NotImplementedError

    def init_b_mps(self):
        raise NotImplementedError

    def oper_prepare(self, omega):
        raise NotImplementedError

    def optimize_cv(self, lr_group, isite, percent=0):
        raise NotImplementedError

    def initialize_LR(self):
        raise NotImplementedError

    def update_LR(self, lr_group, isite):
        raise NotImplementedError
