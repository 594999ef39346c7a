#!/usr/bin/env python3
"""Captures tests/golden/spectral_function_zt.npz from the real reference.  No GPU is needed.

Runs the reference's own ``SpectralFunctionZT`` (transport/spectral_function.py) on the model of
tests/test_spectral_function_gpu.py - a ``TI1DModel`` of 3 cells, each a simple electron and an oscillator with 3 levels,
Holstein coupling g = 0.7 at omega = 1, hopping 0.5, TDVP-PS, 5 steps of 0.5 - and stores what it dumps plus the bond
dimensions of the ket and the deviation of the reference's G from dense propagation.  Only data is written.  The
reference is imported as oracle/gen_golden.py imports it: its checkout and the stand-in modules of oracle/shims on
sys.path.  The checkout is the one oracle/gen_golden.py uses; give its directory as the argument, or in
RENO_REFERENCE_DIR:

    python tools/capture_spectral_function.py REFERENCE_DIR
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("RENO_NUM_THREADS", "4")
os.environ.setdefault("RENO_LOG_LEVEL", "40")
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RENO_REFERENCE_DIR")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "renormalizer")):
    sys.exit("usage: capture_spectral_function.py REFERENCE_DIR (the reference's checkout, or RENO_REFERENCE_DIR)")
sys.path.insert(0, os.path.abspath(REFERENCE))
sys.path.insert(0, os.path.join(REPO, "oracle", "shims"))

import numpy as np  # noqa: E402

OMEGA, G, HOP, NCELL, NLEVEL, NSTEPS, TIME = 1.0, 0.7, 0.5, 3, 3, 5, 2.5


def main():
    import scipy.linalg
    from renormalizer.model import Op, TI1DModel
    from renormalizer.model.basis import BasisSHO, BasisSimpleElectron
    from renormalizer.mps import Mpo
    from renormalizer.transport.spectral_function import SpectralFunctionZT
    from renormalizer.utils import CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod

    basis = [BasisSimpleElectron("e"), BasisSHO("ph", OMEGA, NLEVEL)]
    local = [Op(r"a^\dagger a", "e", G ** 2 * OMEGA), Op(r"b^\dagger b", "ph", OMEGA),
             -G * OMEGA * Op(r"a^\dagger a", "e") * Op(r"b^\dagger + b", "ph")]
    hopping = [Op(r"a^\dagger a", [(0, "e"), (1, "e")], HOP), Op(r"a^\dagger a", [(1, "e"), (0, "e")], HOP)]
    model = TI1DModel(basis, local, hopping, NCELL)
    job = SpectralFunctionZT(model, CompressConfig(CompressCriteria.fixed, max_bonddim=64),
                             EvolveConfig(EvolveMethod.tdvp_ps))
    job.evolve(nsteps=NSTEPS, evolve_time=TIME)
    dump = job.get_dump_dict()
    g_ref = np.asarray(dump["G array"])

    # dense propagation: G_i(t) = -i <gs| a_i exp(-i (H - E0) t) a_0^+ |gs>
    h = Mpo(model).todense()
    gs = np.zeros(h.shape[0])
    gs[0] = 1.0
    e0 = gs @ h @ gs
    a = [Mpo.onsite(model, "a", dof_set={dof}).todense() for dof in model.e_dofs]
    ket0 = a[0].T.conj() @ gs
    times = np.asarray(dump["time series"], dtype=float)
    dense = np.array([[-1j * (gs @ ai @ scipy.linalg.expm(-1j * (h - e0 * np.eye(len(h))) * t) @ ket0) for ai in a]
                      for t in times])
    dev = float(np.abs(g_ref - dense).max())
    print(f"reference G against dense propagation: {dev:.2e}; ket bonds {list(job.latest_mps[1].bond_dims)}")
    out = os.path.join(REPO, "tests", "golden", "spectral_function_zt.npz")
    np.savez_compressed(out, **{"G array": g_ref, "Gk array": np.asarray(dump["Gk array"]),
                                "electron occupations array": np.asarray(dump["electron occupations array"]),
                                "time series": times, "ket bond dims": np.asarray(job.latest_mps[1].bond_dims),
                                "reference deviation from dense": np.array(dev)})
    print("wrote", out)


if __name__ == "__main__":
    main()
