"""Charge-transport jobs (counterpart of renormalizer/transport/).

``TransportKubo`` is the Green-Kubo mobility: the current-current correlation function of a thermal state, one
``<bra| j |ket>`` of two density operators per recorded step (``Mps.matrix_element``, one engine call,
``mpse_mps_sandwich``).  ``ChargeDiffusionDynamics`` and the spectral-function driver are not provided."""
from .kubo import TransportKubo, current_operators

__all__ = ["TransportKubo", "current_operators"]
