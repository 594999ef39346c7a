#!/usr/bin/env python3
"""Aggregate site-updates/s of B disorder realisations of one model on one MI355X: (a) the B states evolved one after
another with Mps.evolve in one thread, (b) evolve_batch (lock-step, batched small-centre Krylov solves).  Config 4 (FMO
thermofield at 77 K, 497 sites, D = 32, as tools/config_times.py builds it, static disorder 50 cm^-1 per seed) and
config 2 (spin-boson, 21 sites, D = 64, coupling alpha scaled per seed).  One JSON line per (config, B, form).
Usage: python tools/batch_bench.py [--configs 4,2] [--batch 1,2,4,8] [--steps K] [--forms seq,batch]"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from renormalizer_amd import (CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, Mpo, Mps,  # noqa: E402
                              Quantity, evolve_batch)
from renormalizer_amd.engine import get_engine  # noqa: E402
from renormalizer_amd.sbm import param2model  # noqa: E402


def config4(seed):
    spec = importlib.util.spec_from_file_location("fmo_example", os.path.join(REPO, "examples", "fmo.py"))
    fmo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fmo)
    model = fmo.fmo_model(35, disorder_cm=50.0, rng=np.random.default_rng(seed), temperature_k=77.0)
    psi = Mpo.onsite(model, r"a^\dagger", dof_set={model.mol_num // 2}).apply(Mps.ground_state(model, False))
    mpo = Mpo(model, offset=Quantity(psi.expectation(Mpo(model))))
    psi.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=32)
    psi.evolve_config = EvolveConfig(EvolveMethod.tdvp_ps)
    return psi.expand_bond_dimension(mpo).canonicalise(), mpo, 160.0


def config2(seed):
    alpha = 0.05 * (1.0 + 0.05 * np.random.default_rng(seed).standard_normal())
    model, _ = param2model(alpha, Quantity(1), Quantity(20), 1, 20, 8)
    mpo = Mpo(model)
    mps = Mps.ground_state(model, False)
    mps.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=64)
    mps.evolve_config = EvolveConfig(EvolveMethod.tdvp_ps)
    return mps.expand_bond_dimension(mpo, coef=1e-16, include_ex=False), mpo, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4,2")
    ap.add_argument("--batch", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms", default="seq,batch")
    a = ap.parse_args()
    eng = get_engine()
    builders = {"4": config4, "2": config2}
    for cfg in a.configs.split(","):
        bmax = max(int(b) for b in a.batch.split(","))
        made = [builders[cfg](seed) for seed in range(bmax)]
        # states of one bond-dimension profile (the lock-step condition): the expansion may differ by seed
        for B in (int(b) for b in a.batch.split(",")):
            states, mpos = [m[0] for m in made[:B]], [m[1] for m in made[:B]]
            dt = made[0][2]
            nsite = len(states[0])
            for form in a.forms.split(","):
                def step(cur):
                    if form == "seq":
                        return [s.evolve(w, dt) for s, w in zip(cur, mpos)]
                    return evolve_batch(cur, mpos, dt)
                cur = list(states)
                for _ in range(a.warmup):
                    cur = step(cur)
                eng.sync()
                b0 = eng.lanczos_batch_stats()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    cur = step(cur)
                eng.sync()
                t = time.perf_counter() - t0
                b1 = eng.lanczos_batch_stats()
                rate = round(2 * nsite * B * a.steps / t, 1) if a.steps else None   # (--steps 0: set-up only, for traces)
                print(json.dumps(dict(config=int(cfg), B=B, form=form, steps=a.steps, sites=nsite,
                                      site_updates_per_s=rate, s_per_step=round(t / a.steps, 4) if a.steps else None, lockstep=len({tuple(s.bond_dims) for s in states}) == 1,
                                      batched_solves=b1[0] - b0[0], single_solves=b1[1] - b0[1])), flush=True)


if __name__ == "__main__":
    main()
