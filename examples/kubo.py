#!/usr/bin/env python3
"""Green-Kubo mobility of a Holstein chain: the current-current correlation function C(t) of the thermal state,
propagated in real time by TDVP-PS, and its integral over k_B T.

    python examples/kubo.py [molecules=5] [steps=20] [bond=24] [temperature_K=50000]

One mode per molecule (omega = 1, displacement 1, 2 levels), J = 1, atomic units; the model of the reference's own Kubo
test.  Prints C(t) after every step, which of the two paths of ``Mps.matrix_element`` the recorded values took, and the
mobility in atomic units and in cm^2 / V s."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from renormalizer_amd import (CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, HolsteinModel, Mol, Phonon,  # noqa: E402
                              Quantity)
from renormalizer_amd.engine import get_engine  # noqa: E402
from renormalizer_amd.transport import TransportKubo  # noqa: E402

nmol = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
bond = int(sys.argv[3]) if len(sys.argv) > 3 else 24
kelvin = float(sys.argv[4]) if len(sys.argv) > 4 else 50000.0

ph = Phonon.simple_phonon(Quantity(1), Quantity(1), 2)
model = HolsteinModel([Mol(Quantity(0), [ph])] * nmol, Quantity(1), 3)
kubo = TransportKubo(model, Quantity(kelvin, "K"),
                     compress_config=CompressConfig(CompressCriteria.fixed, max_bonddim=bond),
                     ievolve_config=EvolveConfig(EvolveMethod.tdvp_ps, adaptive=True, guess_dt=-0.1j),
                     evolve_config=EvolveConfig(EvolveMethod.tdvp_ps, adaptive=True, guess_dt=0.5, adaptive_rtol=1e-3))
kubo.evolve(evolve_dt=0.5, nsteps=steps)

print("      t        Re C(t)        Im C(t)")
for t, c in zip(kubo.evolve_times, kubo.auto_corr):
    print(f"{t:7.2f}  {c.real:13.6e}  {c.imag:13.6e}")
stats = get_engine().mps_sandwich_stats()
print(f"matrix elements: {stats['chain_kernel']} through the chain kernel, {stats['enqueued']} through enqueued updates")
au, cm2 = kubo.calc_mobility()
tail = np.abs(kubo.auto_corr[-3:]).max() / np.abs(kubo.auto_corr[0])
print(f"mobility {au:.6e} a.u. = {cm2:.6e} cm^2/Vs  (|C| at the end of the window: {tail:.1e} of C(0))")
