"""Charge-transport jobs (counterpart of renormalizer/transport/).

``TransportKubo`` is the Green-Kubo mobility: the current-current correlation function of a thermal state, one
``<bra| j |ket>`` of two density operators per recorded step (``Mps.matrix_element``, one engine call,
``mpse_mps_sandwich``).  ``ChargeDiffusionDynamics`` is the real-time diffusion of an electron created on the centre
molecule, at zero or finite temperature; with ``rdm=True`` it records the reduced density matrix of the electron after
every step, which is ``Mps.edof_rdm()``: one walk over the chain inside the engine (``mpse_mps_corr``).
``SpectralFunctionZT`` is the zero-temperature one-particle Green's function G_i(t) = <gs| a_i |ket(t)> / 1j of a
translationally invariant chain; every recorded row is ``Mps.transition_elements``: one walk over the two chains inside
the engine (``mpse_mps_trdm1``)."""
from .dynamics import EDGE_THRESHOLD, ChargeDiffusionDynamics, InitElectron, calc_r_square
from .kubo import TransportKubo, current_operators
from .spectral_function import SpectralFunctionZT

__all__ = ["TransportKubo", "current_operators", "ChargeDiffusionDynamics", "InitElectron", "EDGE_THRESHOLD",
           "calc_r_square", "SpectralFunctionZT"]
