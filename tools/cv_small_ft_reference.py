"""Writes tests/golden/cv_small_ft_exact.npz: the reference's SpectraFtCV on a model small enough for dense algebra,
next to the exact finite-temperature resolvent.

    python tools/cv_small_ft_reference.py /path/to/Renormalizer

Development machines only (imports the reference package from the given checkout, CPU); no GPU test needs this script,
only the fixture it writes.  Model: that of tests/golden/cv_small_exact.npz (2 molecules x 1 mode of 1555.55 cm^-1 with
4 levels) at 600 K, where the second vibrational level holds 2.3 % of the weight (at room temperature: 0.05 %).
Absorption, m_max = 64 (above every exact bond dimension of the |1><0| sector: truncation plays no part).  The dense
value is defined from b itself, so that no normalisation convention enters: B = b_mpo.todense() restricted to the
sector of operators |one exciton><no exciton|, A = (omega - Liou)^2 + eta^2 with Liou X = H X - X H on that sector,
value = <B| A^-1 |B> / (pi eta).  Five frequencies: the two strongest maxima of the dense spectrum, the point half way
between them, one point in each tail.  Stored: omega, the reference's results, the dense values and the reference's
relative deviation from them, per frequency; temperature, eta, m_max, rtol and the model parameters.  A frequency at
which the reference itself misses the dense value by more than its sweep rtol is a bad yardstick and has to be moved:
the script says so and writes nothing."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

ETA, M_MAX, RTOL, T_K = 5.0e-4, 64, 1.0e-5, 600.0
PARAMS = dict(elocalex_ev=2.67, dipole=15.45, omega_cm=1555.55, displacement=8.7729, levels=4, j_ev=-0.1, nmols=2)


def sector_problem(h, nex, b):
    """(Liouvillian on the |1><0| sector as a matrix on row-major vec(X), vec(B)) from dense H, the exciton number of
    every basis state and dense B"""
    r, c = np.nonzero(nex == 1)[0], np.nonzero(nex == 0)[0]
    h11, h00 = h[np.ix_(r, r)], h[np.ix_(c, c)]
    liou = np.kron(h11, np.eye(len(c))) - np.kron(np.eye(len(r)), h00.T)
    bs = b[np.ix_(r, c)]
    outside = np.abs(b).sum() - np.abs(bs).sum()
    assert outside < 1e-12 * np.abs(b).sum(), "b leaves the sector"
    return liou, bs.ravel()


def dense_value(liou, vb, omega, eta):
    m = omega * np.eye(len(liou)) - liou
    a = m @ m + eta * eta * np.eye(len(liou))
    return float(np.vdot(vb, np.linalg.solve(a, vb)).real / (np.pi * eta))


def main():
    ref = sys.argv[1]
    sys.path.insert(0, os.path.join(REPO, "oracle", "shims"))
    sys.path.insert(0, ref)
    from renormalizer.cv import batch_run
    from renormalizer.cv.finitet import SpectraFtCV
    from renormalizer.model import HolsteinModel, Mol, Phonon
    from renormalizer.mps import Mpo
    from renormalizer.utils import Quantity, constant

    # scipy.sparse.linalg.cg(tol=...) is the argument's name up to SciPy 1.11; later releases call it rtol
    import inspect
    import scipy.sparse.linalg
    cg = scipy.sparse.linalg.cg
    if "tol" not in inspect.signature(cg).parameters:
        scipy.sparse.linalg.cg = lambda a, b, tol=1e-5, **kw: cg(a, b, rtol=tol, **kw)

    p = PARAMS
    ph = Phonon.simple_phonon(Quantity(p["omega_cm"], "cm^{-1}"), Quantity(p["displacement"]), p["levels"])
    j = np.array([[0.0, p["j_ev"]], [p["j_ev"], 0.0]]) / constant.au2ev
    model = HolsteinModel([Mol(Quantity(p["elocalex_ev"], "eV"), [ph], p["dipole"])] * p["nmols"], j)
    temperature = Quantity(T_K, "K")
    x = p["omega_cm"] / (temperature.as_au() / Quantity(1, "cm^{-1}").as_au())
    pop1 = np.exp(-x) * (1 - np.exp(-x))
    print(f"population of the second vibrational level at {T_K} K: {pop1:.4f}")
    assert pop1 >= 0.01
    h_mpo = Mpo(model, offset=Quantity(model.gs_zpe))
    spectra = SpectraFtCV(model, "abs", M_MAX, ETA, temperature, h_mpo, rtol=RTOL)
    h = np.asarray(h_mpo.todense())
    nex = np.rint(np.diag(np.asarray(Mpo.onsite(model, r"a^\dagger a").todense())).real).astype(int)
    liou, vb = sector_problem(h, nex, np.asarray(spectra.b_mpo.todense()))
    # the spectrum on a grid from the eigenbasis of the (Hermitian) Liouvillian
    lw, lv = np.linalg.eigh((liou + liou.conj().T) / 2)
    grid = np.arange(lw.min() - 40 * ETA, lw.max() + 40 * ETA, ETA / 4)
    wgt = np.abs(lv.conj().T @ vb) ** 2
    spec = np.array([(wgt / ((w - lw) ** 2 + ETA ** 2)).sum() for w in grid]) / (np.pi * ETA)
    peaks = [k for k in range(1, len(grid) - 1) if spec[k] > spec[k - 1] and spec[k] >= spec[k + 1]]
    peaks = sorted(sorted(peaks, key=lambda k: -spec[k])[:2])
    w1, w2 = grid[peaks[0]], grid[peaks[1]]
    lines = lw[wgt > 1e-8 * wgt.max()]
    omega = np.array([lines.min() - 30 * ETA, w1, 0.5 * (w1 + w2), w2, lines.max() + 30 * ETA])
    exact = np.array([dense_value(liou, vb, w, ETA) for w in omega])
    res = np.array(batch_run(omega.tolist(), 1, spectra), dtype=float)
    dev = np.abs(res - exact) / np.abs(exact)
    for w, a, b, d in zip(omega, res, exact, dev):
        print(f"omega {w:.6f}  reference {a:.8e}  dense {b:.8e}  relative deviation {d:.2e}")
    if np.any(dev > RTOL):
        print("the reference misses the dense value by more than its sweep rtol: move that frequency")
        sys.exit(1)
    out = os.path.join(REPO, "tests", "golden", "cv_small_ft_exact.npz")
    np.savez(out, omega=omega, reference=res, dense=exact, reference_rel_dev=dev, eta=ETA, m_max=M_MAX, rtol=RTOL,
             temperature_k=T_K, second_level_population=pop1, **{k: np.asarray(val) for k, val in p.items()})
    print("wrote", out)


if __name__ == "__main__":
    main()
