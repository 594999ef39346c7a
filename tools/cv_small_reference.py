"""Writes tests/golden/cv_small_exact.npz: the reference's SpectraZtCV on a model small enough for dense algebra, next
to the exact resolvent.

    python tools/cv_small_reference.py /path/to/Renormalizer

Development machines only (imports the reference package from the given checkout, CPU); no GPU test needs this script,
only the fixture it writes.  Model: 2 molecules x 1 mode with 4 levels (64 states, 32 in the one-exciton sector),
absorption from the vibrational ground state, m_max = 16 (above every exact bond dimension of the sector: truncation
plays no part).  Five frequencies: the two strongest peaks, one point between them, one in each tail.  Stored: omega,
the reference's results, the dense values -(1/pi) Im <psi0| mu^+ (omega + e0 - H + i eta)^-1 mu |psi0> and the
reference's relative deviation from them, per frequency; eta, m_max, rtol and the model parameters."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

ETA, M_MAX, RTOL = 5.0e-4, 16, 1.0e-5
PARAMS = dict(elocalex_ev=2.67, dipole=15.45, omega_cm=1555.55, displacement=8.7729, levels=4, j_ev=-0.1, nmols=2)


def main():
    ref = sys.argv[1]
    sys.path.insert(0, os.path.join(REPO, "oracle", "shims"))
    sys.path.insert(0, ref)
    from renormalizer.cv import batch_run
    from renormalizer.cv.zerot import SpectraZtCV
    from renormalizer.model import HolsteinModel, Mol, Phonon
    from renormalizer.mps import Mpo
    from renormalizer.utils import Quantity, constant

    # the reference calls scipy.sparse.linalg.cg(tol=...), the name of that argument up to SciPy 1.11; later releases
    # call it rtol (same meaning with atol = 0, which the reference passes)
    import inspect
    import scipy.sparse.linalg
    cg = scipy.sparse.linalg.cg
    if "tol" not in inspect.signature(cg).parameters:
        scipy.sparse.linalg.cg = lambda a, b, tol=1e-5, **kw: cg(a, b, rtol=tol, **kw)

    p = PARAMS
    ph = Phonon.simple_phonon(Quantity(p["omega_cm"], "cm^{-1}"), Quantity(p["displacement"]), p["levels"])
    j = np.array([[0.0, p["j_ev"]], [p["j_ev"], 0.0]]) / constant.au2ev
    model = HolsteinModel([Mol(Quantity(p["elocalex_ev"], "eV"), [ph], p["dipole"])] * p["nmols"], j)
    h = np.asarray(Mpo(model).todense())
    mu = np.asarray(Mpo.onsite(model, r"a^\dagger", dipole=True).todense())
    ew, ev = np.linalg.eigh(h)
    e0, psi0 = ew[0], ev[:, 0]
    v = mu @ psi0
    weight = np.abs(ev.conj().T @ v) ** 2
    lines = ew - e0
    strong = np.argsort(weight)[::-1][:2]
    w1, w2 = sorted(lines[strong])
    omega = np.array([w1 - 30 * ETA, w1, 0.5 * (w1 + w2), w2, lines[weight > 1e-8 * weight.max()].max() + 30 * ETA])

    def dense(w):
        g = np.linalg.solve((w + e0) * np.eye(len(h)) - h + 1j * ETA * np.eye(len(h)), v)
        return -np.vdot(v, g).imag / np.pi

    exact = np.array([dense(w) for w in omega])
    spectra = SpectraZtCV(model, "abs", M_MAX, ETA, rtol=RTOL)
    res = np.array(batch_run(omega.tolist(), 1, spectra), dtype=float)
    dev = np.abs(res - exact) / np.abs(exact)
    for w, a, b, d in zip(omega, res, exact, dev):
        print(f"omega {w:.6f}  reference {a:.8e}  dense {b:.8e}  relative deviation {d:.2e}")
    out = os.path.join(REPO, "tests", "golden", "cv_small_exact.npz")
    np.savez(out, omega=omega, reference=res, dense=exact, reference_rel_dev=dev, eta=ETA, m_max=M_MAX, rtol=RTOL,
             e0=e0, **{k: np.asarray(val) for k, val in p.items()})
    print("wrote", out)


if __name__ == "__main__":
    main()
