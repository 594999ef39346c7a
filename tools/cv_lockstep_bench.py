#!/usr/bin/env python3
"""Wall time of a 16-point zero-temperature absorption grid (the model of examples/cv_abs.py): serial ``cv.batch_run``
against ``cv.batch_run_lockstep`` at widths 1, 4 and 8, the runs alternated, several passes each (every run starts from
the same ground state and the same start vector).  Prints one JSON line per run.

    python tools/cv_lockstep_bench.py [passes=3]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity  # noqa: E402
from renormalizer_amd.cv import SpectraZtCV, batch_run, batch_run_lockstep  # noqa: E402
from renormalizer_amd.engine import get_engine  # noqa: E402
from renormalizer_amd.mps.mps import Mps  # noqa: E402
from renormalizer_amd.utils import constant  # noqa: E402

passes = int(sys.argv[1]) if len(sys.argv) > 1 else 3
omega = [Quantity(106.51, "cm^{-1}"), Quantity(1555.55, "cm^{-1}")]
dis = [Quantity(30.1370), Quantity(8.7729)]
ph_list = [Phonon.simple_phonon(o, d, 4) for o, d in zip(omega, dis)]
j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list, 15.45)] * 3, j, 3)
eng = get_engine()
freq = np.linspace(0.0835, 0.0845, 16).tolist()
first = SpectraZtCV(model, "abs", 10, 5.0e-5, rtol=1e-3)
start = Mps.random(model, first.b_mps.qntot, 10, percent=1.0, rng=np.random.default_rng(5))


def job():
    return SpectraZtCV(model, "abs", 10, 5.0e-5, rtol=1e-3, b_mps=first.b_mps, e0=first.e0, cv_mps=start.copy())


def timed(fn):
    eng.sync()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return time.perf_counter() - t0, out


runs = {"serial": lambda: batch_run(freq, 1, job())}
for w in (1, 4, 8):
    runs[f"lockstep{w}"] = (lambda w=w: batch_run_lockstep(freq, job(), width=w))
for fn in runs.values():       # warm-up: allocator pool, code objects
    fn()
times = {k: [] for k in runs}
for _ in range(passes):
    for k, fn in runs.items():
        times[k].append(timed(fn)[0])
for k, v in times.items():
    print(json.dumps({"run": k, "points": len(freq), "seconds": [round(x, 4) for x in v],
                      "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}))
