#!/usr/bin/env python3
"""Tangent-space (TDA) excited states on top of a DMRG ground state: the 3-molecule Holstein model with two modes per
molecule (3 and 2 phonon levels), one exciton, M = 8 (mps/tda.py of the reference).

The Hamiltonian is shifted by the ground-state energy, so the roots are excitation energies of the reference state.
Note that TDA ignores quantum numbers, like the reference: the tangent space of a one-exciton state also reaches the
zero-exciton sector, whose vacuum lies BELOW the one-exciton ground state by its excitation energy.  The lowest root
is therefore negative - the zero-point energy minus the offset, about -0.084 Hartree (the reference's TDA returns the
same kind of root for this model) - and the roots that follow are phonon excitations of that sector."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity  # noqa: E402
from renormalizer_amd.mps import TDA, Mps  # noqa: E402
from renormalizer_amd.mps.gs import optimize_mps  # noqa: E402
from renormalizer_amd.utils import constant  # noqa: E402

M = 8
ph_list = [Phonon.simple_phonon(Quantity(106.51, "cm^{-1}"), Quantity(30.1370), 3),
           Phonon.simple_phonon(Quantity(1555.55, "cm^{-1}"), Quantity(8.7729), 2)]
j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list)] * 3, j, 3)

mps = Mps.random(model, 1, M, rng=np.random.default_rng(2024))
mps.optimize_config.procedure = [[M, 0.4], [M, 0.2], [M, 0.1], [M, 0], [M, 0]]
mps.optimize_config.method = "2site"
energies, mps = optimize_mps(mps, Mpo(model))
e_gs = min(energies)
print(f"ground state of the one-exciton sector: {e_gs:.8f} (zero-point energy {model.gs_zpe:.8f})")

np.random.seed(1)
tda = TDA(model, Mpo(model, offset=Quantity(e_gs)), mps, nroots=3)
e = tda.kernel(include_psi0=True)
print("TDA roots relative to the ground state:", e)
print(f"lowest root {e[0]:.8f}, zero-point energy minus offset {model.gs_zpe - e_gs:.8f}")
print(f"{tda.ncycle} Davidson cycles, {tda.nmatvec} applications of the projected Hamiltonian")
