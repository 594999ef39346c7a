"""Time-domain spectra, counterpart of renormalizer/spectra/: one propagation of the dipole autocorrelation function
C(t) = <bra(t)|ket(t)>, whose Fourier transform is the absorption / emission spectrum.

Every job is a ``TdMpsJob`` whose state is a ``BraKetPair``; after each step the pair's overlap is taken by
``Mps.overlap`` (one engine call, ``mpse_mps_overlap``) and recorded in ``autocorr``.  The states are prepared and
propagated with the parts the other drivers use: ``optimize_mps``, ``Mpo.onsite(..., dipole=True).apply``,
``expand_bond_dimension``, ``Mps.evolve``, ``evolve_exact``, ``thermal_state`` and ``MpDm``."""
from .base import SpectraTdMpsJobBase
from .exact import SpectraExact
from .finitet import BraKetPairAbsFiniteT, BraKetPairEmiFiniteT, SpectraFiniteT
from .zerot import SpectraOneWayPropZeroT, SpectraTwoWayPropZeroT, SpectraZeroT

__all__ = ["SpectraTdMpsJobBase", "SpectraExact", "SpectraZeroT", "SpectraOneWayPropZeroT", "SpectraTwoWayPropZeroT",
           "SpectraFiniteT", "BraKetPairAbsFiniteT", "BraKetPairEmiFiniteT"]
