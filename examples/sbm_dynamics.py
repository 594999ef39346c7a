#!/usr/bin/env python3
"""Spin-boson dynamics at zero temperature with the job of the reference, ``SpinBosonDynamics`` (renormalizer/sbm):
Ohmic bath, adiabatically renormalised tunnelling, spin up, bath in its vacuum, TDVP-PS at a fixed bond dimension from
the padded product state.  Per step the job records <sigma_x>, <sigma_z>, the spin's density matrix and the entropy of
every bond, the last two from one engine call each (``Mps.site_rdms``, ``Mps.bond_entropies``).

    python examples/sbm_dynamics.py [n_phonons=20] [nsteps=20] [bond=64] [dump_dir]

With a fourth argument the series go to <dump_dir>/sbm.npz after every step.  examples/sbm.py is the same model as a
hand-written loop."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from renormalizer_amd import CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, Quantity  # noqa: E402
from renormalizer_amd.sbm import SpinBosonDynamics, param2mollist  # noqa: E402


if __name__ == "__main__":
    n_phonons = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    bond = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    dump_dir = sys.argv[4] if len(sys.argv) > 4 else None
    model = param2mollist(alpha=0.05, raw_delta=Quantity(1), omega_c=Quantity(20), renormalization_p=1, n_phonons=n_phonons)
    job = SpinBosonDynamics(model, compress_config=CompressConfig(CompressCriteria.fixed, max_bonddim=bond),
                            evolve_config=EvolveConfig(EvolveMethod.tdvp_ps), dump_dir=dump_dir,
                            job_name="sbm" if dump_dir else None)
    job.evolve(evolve_dt=0.1, nsteps=nsteps)
    for t, sz, sx, s in zip(job.evolve_times, job.sigma_z, job.sigma_x, job.bond_entropy):
        print(f"t = {t:6.2f}  <sigma_z> = {sz:+.8f}  <sigma_x> = {sx:+.8f}  largest bond entropy = {max(s):.6f}")
