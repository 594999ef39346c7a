"""Purified thermal state by imaginary-time propagation (the preparer behind the reference's finite-temperature
runs, mps/thermalprop.py:95-133): rho(beta/2) = exp(-beta H / 2) rho(0), ``nsteps`` calls of ``MpDm.evolve`` with an
imaginary step, the Hamiltonian re-referenced to the latest energy before every step so the norm stays O(1).
``thermal_state`` is the bare loop; ``ThermalProp`` is the reference's job around it, which records the energy, the
occupations, the bond entropies and the user's ``Property`` after every step and dumps them."""
import logging

import numpy as np

from ..utils import Quantity
from ..utils.tdmps import TdMpsJob
from .mpo import Mpo

logger = logging.getLogger("renormalizer_amd")


def thermal_state(init_mpdm, h_mpo, evolve_dt, nsteps, auto_expand=True, on_step=None):
    """Returns (rho(beta / 2), energies).  ``evolve_dt`` = beta / 2j / nsteps (negative imaginary); ``on_step(rho)`` is
    called on the initial state and after every step."""
    assert np.iscomplex(evolve_dt) and np.imag(evolve_dt) < 0
    rho = init_mpdm.canonicalise()
    if rho.evolve_config.is_tdvp and auto_expand:
        rho = rho.expand_bond_dimension(h_mpo)
    energies = [rho.expectation(h_mpo)]
    if on_step is not None:
        on_step(rho)
    for _ in range(nsteps):
        rho = rho.evolve(Mpo(h_mpo.model, offset=Quantity(energies[-1])), evolve_dt)
        energies.append(rho.expectation(h_mpo))
        if on_step is not None:
            on_step(rho)
    return rho, energies


class ThermalProp(TdMpsJob):
    """Imaginary-time propagation of a density operator as a job (mps/thermalprop.py:13-148).

    init_mpdm: the initial ``MpDm``, usually the identity; h_mpo_model: the model of the Hamiltonian (default: that of
    ``init_mpdm``); exact: the Hamiltonian is a sum of one-site vibrational terms and every step is the product of
    local exponentials ``Mpo.exact_propagator`` in the space ``space`` ("GS": no exciton, "EX": one exciton, displaced
    oscillators) - occupations, entropies and properties are then not recorded; evolve_config: of the propagation;
    dump_mps / dump_dir / job_name: as ``TdMpsJob``; properties: a ``Property`` whose ``calc_properties`` is called
    after every step; auto_expand: widen the bonds of the initial state before a TDVP propagation."""

    def __init__(self, init_mpdm, h_mpo_model=None, exact: bool = False, space: str = "GS", evolve_config=None,
                 dump_mps=None, dump_dir: str = None, job_name: str = None, properties=None, auto_expand: bool = True):
        self.init_mpdm = init_mpdm.canonicalise()
        if h_mpo_model is None:
            h_mpo_model = self.init_mpdm.model
        self.h_mpo = Mpo(h_mpo_model)
        logger.info(f"bond dims of h_mpo {self.h_mpo.bond_dims}")
        self.exact = exact
        assert space in ["GS", "EX"]
        self.space = space
        self.energies = []
        self._e_occupations_array = []
        self._ph_occupations_array = []
        self._vn_entropy_array = []
        self.properties = properties
        self.auto_expand = auto_expand
        super().__init__(evolve_config=evolve_config, dump_mps=dump_mps, dump_dir=dump_dir, job_name=job_name)

    def init_mps(self):
        self.init_mpdm.evolve_config = self.evolve_config
        if self.evolve_config.is_tdvp and self.auto_expand:
            self.init_mpdm = self.init_mpdm.expand_bond_dimension(self.h_mpo)
        return self.init_mpdm

    def process_mps(self, mps):
        energy = mps.expectation(self.h_mpo)
        self.energies.append(energy)
        if self.exact:
            return
        self._e_occupations_array.append(mps.e_occupations)
        self._ph_occupations_array.append(mps.ph_occupations)
        self._vn_entropy_array.append(mps.calc_bond_entropy())
        logger.info(f"energy {energy}, electrons {self._e_occupations_array[-1].sum()}")
        if self.properties is not None:
            self.properties.calc_properties(mps)

    def evolve_exact(self, old_mpdm, evolve_dt):
        prop = Mpo.exact_propagator(old_mpdm.model, evolve_dt.imag, space=self.space, shift=-self.energies[-1])
        new_mpdm = prop.apply(old_mpdm, canonicalise=True)
        # the partition function is out of reach: it does not fit a float
        new_mpdm.normalize("mps_and_coeff")
        return new_mpdm

    def evolve_prop(self, old_mpdm, evolve_dt):
        """one step with the Hamiltonian re-referenced to the latest energy, so the norm stays O(1)"""
        return old_mpdm.evolve(Mpo(self.h_mpo.model, offset=Quantity(self.energies[-1])), evolve_dt)

    def evolve_single_step(self, evolve_dt):
        step = self.evolve_exact if self.exact else self.evolve_prop
        return step(self.latest_mps, evolve_dt)

    def evolve(self, evolve_dt=None, nsteps=None, evolve_time=None):
        if evolve_dt is not None:
            assert np.iscomplex(evolve_dt) and evolve_dt.imag < 0
        if evolve_time is not None:
            assert np.iscomplex(evolve_time) and evolve_time.imag < 0
        return super().evolve(evolve_dt, nsteps, evolve_time)

    @property
    def e_occupations_array(self):
        return np.array(self._e_occupations_array)

    @property
    def ph_occupations_array(self):
        return np.array(self._ph_occupations_array)

    @property
    def vn_entropy_array(self):
        return np.array(self._vn_entropy_array)

    def get_dump_dict(self):
        dump = {"time series": [-np.imag(t) for t in self.evolve_times], "energies": self.energies,
                "electron occupations array": self.e_occupations_array.tolist(),
                "phonon occupations array": self.ph_occupations_array.tolist(),
                "vn entropy array": self.vn_entropy_array.tolist()}
        if self.properties is not None:
            for name, res in self.properties.prop_res.items():
                dump[name] = res
        return dump
