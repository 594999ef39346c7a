"""Frequency-domain spectra by the correction vector (dynamical DMRG), counterpart of renormalizer/cv/.

Zero temperature only (``SpectraZtCV``): the centre problems ((H - e0 - omega)^2 + eta^2) x = b are solved inside the
engine by ``mpse_pcg`` (include/mpsengine.h)."""
from .spectra_cv import SpectraCv, batch_run
from .zerot import SpectraZtCV

__all__ = ["SpectraCv", "SpectraZtCV", "batch_run"]
