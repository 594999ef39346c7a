#!/usr/bin/env python3
"""One-particle Green's function of a Holstein ring with ``SpectralFunctionZT``: a translationally invariant chain of
``ncell`` cells, each one electronic level coupled to one oscillator, nearest-neighbour hopping with a periodic
boundary; the electron is created on the first cell and the ket is propagated by TDVP-PS at a fixed bond dimension.
After every step the job records G_i(t) = <gs| a_i |ket(t)> / 1j for every cell (``Mps.transition_elements``: one engine
call) and the example prints its k-space transform G_k(t) = sum_d G_d(t) exp(i k d) for k = 0 .. pi.

    python examples/spectral_function.py [ncell=6] [nlevel=4] [D=32] [nsteps=10] [dt=0.5] [g=0.7] [hopping=0.5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from renormalizer_amd import CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, Op  # noqa: E402
from renormalizer_amd.engine import get_engine  # noqa: E402
from renormalizer_amd.model.basis import BasisSHO, BasisSimpleElectron  # noqa: E402
from renormalizer_amd.model.model import TI1DModel  # noqa: E402
from renormalizer_amd.transport import SpectralFunctionZT  # noqa: E402


def main():
    defaults = [6, 4, 32, 10, 0.5, 0.7, 0.5]
    given = sys.argv[1:8]
    ncell, nlevel, D, nsteps = [int(a) for a in given[:4]] + defaults[len(given[:4]):4]
    dt, g, hop = [float(a) for a in given[4:7]] + defaults[4 + len(given[4:7]):7]
    omega = 1.0
    basis = [BasisSimpleElectron("e"), BasisSHO("ph", omega, nlevel)]
    local = [Op(r"a^\dagger a", "e", g ** 2 * omega), Op(r"b^\dagger b", "ph", omega),
             -g * omega * Op(r"a^\dagger a", "e") * Op(r"b^\dagger + b", "ph")]
    hopping = [Op(r"a^\dagger a", [(0, "e"), (1, "e")], hop), Op(r"a^\dagger a", [(1, "e"), (0, "e")], hop)]
    model = TI1DModel(basis, local, hopping, ncell)
    job = SpectralFunctionZT(model, CompressConfig(CompressCriteria.fixed, max_bonddim=D),
                             EvolveConfig(EvolveMethod.tdvp_ps))
    job.evolve(evolve_dt=dt, nsteps=nsteps)
    dump = job.get_dump_dict()
    gk = np.asarray(dump["Gk array"])
    ks = np.arange(gk.shape[1]) * 2 / ncell
    print("t      " + "  ".join(f"G_k(t), k = {k:4.2f} pi     " for k in ks))
    for t, row in zip(job.evolve_times, gk):
        print(f"{t:5.2f}  " + "  ".join(f"{v.real:+10.6f} {v.imag:+10.6f} i" for v in row))
    stats = get_engine().mps_trdm1_stats()
    print(f"ket bond dimensions {list(job.latest_mps[1].bond_dims)}")
    print(f"mpse_mps_trdm1: {stats['chain_kernel']} calls through the chain kernels, {stats['enqueued']} through the "
          f"enqueued products, {stats['matrices']} matrices")


if __name__ == "__main__":
    main()
