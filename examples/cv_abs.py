#!/usr/bin/env python3
"""Zero-temperature absorption spectrum of a Holstein trimer in the frequency domain (correction vector / DDMRG):
the reference's cv/tests/test_abs.py model over a window around its strongest line, printed as two columns
(frequency in a.u., spectral value).

    python examples/cv_abs.py [points=9] [width=0]

width > 0: the frequencies run in lock-step, ``width`` at a time (cv.batch_run_lockstep; every frequency then starts
from the same random correction vector instead of its predecessor's result)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity  # noqa: E402
from renormalizer_amd.cv import SpectraZtCV, batch_run, batch_run_lockstep  # noqa: E402
from renormalizer_amd.utils import constant  # noqa: E402

points = int(sys.argv[1]) if len(sys.argv) > 1 else 9
width = int(sys.argv[2]) if len(sys.argv) > 2 else 0
omega = [Quantity(106.51, "cm^{-1}"), Quantity(1555.55, "cm^{-1}")]
dis = [Quantity(30.1370), Quantity(8.7729)]
ph_list = [Phonon.simple_phonon(o, d, 4) for o, d in zip(omega, dis)]
j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list, 15.45)] * 3, j, 3)

eta = 5.0e-5
freq = np.linspace(0.0835, 0.0845, points)
spectra = SpectraZtCV(model, "abs", 10, eta, rtol=1e-3)
values = batch_run_lockstep(freq.tolist(), spectra, width=width) if width > 0 else batch_run(freq.tolist(), 1, spectra)
for w, s in zip(freq, values):
    print(f"{w:.6f}  {s:.6e}")
