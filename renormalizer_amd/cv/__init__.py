"""Frequency-domain spectra by the correction vector (dynamical DMRG), counterpart of renormalizer/cv/.

Zero temperature (``SpectraZtCV``): the centre problems ((H - e0 - omega)^2 + eta^2) x = b are solved inside the engine
by ``mpse_pcg``.  Finite temperature (``SpectraFtCV``): the correction vector is an operator, the centre problems
((omega - Liou)^2 + eta^2) x = b are a sum of three two-layer terms solved by ``mpse_pcg_sum`` (include/mpsengine.h).
``batch_run_lockstep`` sweeps several zero-temperature frequencies together, their centre systems in one
``mpse_pcg_batch`` call per site."""
from .finitet import SpectraFtCV
from .lockstep import batch_run_lockstep
from .spectra_cv import SpectraCv, batch_run
from .zerot import SpectraZtCV

__all__ = ["SpectraCv", "SpectraFtCV", "SpectraZtCV", "batch_run", "batch_run_lockstep"]
