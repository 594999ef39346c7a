#!/usr/bin/env python3
"""Writes tests/golden/tda_holstein_small.npz from the reference implementation (development machines only: it imports
the ``renormalizer`` package, which must be on PYTHONPATH together with the stand-in modules of oracle/shims):

    PYTHONPATH=oracle/shims:<reference checkout> python tools/gen_tda_golden.py

The 3-molecule Holstein model of tests/test_model_mpo.py: ground state of the one-exciton sector by the reference's
``optimize_mps`` at M = 8 from a seeded random state, then the reference's ``TDA`` (``algo="davidson"``, ``nroots = 4``,
seeded NumPy guess) for both ``include_psi0`` settings.  One ``kernel()`` call does not converge on this model: three
identical molecules put eigenvalues of the projected Hamiltonian 8e-7 apart and the iteration runs out of its 100
cycles with energies 3e-8 to 3e-6 above the eigenvalues.  So the call is continued with the reference's own
``kernel(restart=True)`` until two successive calls return the same energies to 1e-12: ``e`` / ``e_psi0`` are those,
``e_first`` / ``e_psi0_first`` what the first call returned, ``restarts`` / ``restarts_psi0`` how many calls followed it.
Stored besides: the optimised state's site arrays and quantum numbers.  Only data is written."""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "tda_holstein_small.npz")
M, NROOTS, SEED, MAX_RESTARTS = 8, 4, 2024, 40


def main():
    from renormalizer.model import HolsteinModel, Mol, Phonon
    from renormalizer.mps import Mpo, Mps, TDA
    from renormalizer.mps.gs import optimize_mps
    from renormalizer.utils import Quantity

    omega = [Quantity(106.51, "cm^{-1}"), Quantity(1555.55, "cm^{-1}")]
    dis = [Quantity(30.1370), Quantity(8.7729)]
    ph_list = [Phonon.simple_phonon(o, d, n) for o, d, n in zip(omega, dis, (3, 2))]
    j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / 27.211386245988
    model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list)] * 3, j, 3)
    mpo = Mpo(model)
    np.random.seed(SEED)
    mps = Mps.random(model, 1, M, percent=1.0)
    mps.optimize_config.procedure = [[M, 0.4], [M, 0.2], [M, 0.1], [M, 0], [M, 0]]
    mps.optimize_config.method = "2site"
    energies, mps = optimize_mps(mps.copy(), mpo)
    data = {"nsites": len(mps), "e_gs": float(np.min(energies)), "qnidx": int(mps.qnidx),
            "qntot": np.asarray(mps.qntot), "to_right": bool(mps.to_right), "m": M, "nroots": NROOTS, "seed": SEED}
    for i, ms in enumerate(mps):
        data[f"mt_{i}"] = np.asarray(ms.array)
    for i, q in enumerate(mps.qn):
        data[f"qn_{i}"] = np.asarray(q)
    for psi0 in (False, True):
        np.random.seed(SEED + 1)
        tda = TDA(model, mpo, mps.copy(), nroots=NROOTS, algo="davidson")
        e = np.asarray(tda.kernel(include_psi0=psi0))
        key = "e_psi0" if psi0 else "e"
        data[key + "_first"] = e
        print("include_psi0 =", psi0, "first call", e)
        for k in range(1, MAX_RESTARTS + 1):
            e_new = np.asarray(tda.kernel(restart=True, include_psi0=psi0))
            done = np.abs(e_new - e).max() < 1e-12
            e = e_new
            if done:
                break
        else:
            raise RuntimeError("the reference's TDA did not become stationary")
        data[key] = e
        data["restarts_psi0" if psi0 else "restarts"] = k
        print("include_psi0 =", psi0, "after", k, "restarts", e)
    np.savez(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
