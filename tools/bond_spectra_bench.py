#!/usr/bin/env python3
"""Times the bond entropies taken after every step, on one GPU: ``Mps.calc_bond_entropy()`` (a copy of the state, a
sweep of blocked QRs into right-canonical form and a sweep of blocked SVDs back, a host read per bond) against
``Mps.bond_entropies()`` (one engine call, ``mpse_mps_bond_spectra``) through the chain kernels
(MPSE_BOND_SPECTRA_CHAIN=1: every chain whose launches fit, also above the bond limit of the path rule, which is read
off this table) and through the enqueued path (MPSE_BOND_SPECTRA_CHAIN=0: products and two block SVDs per bond).

    python tools/bond_spectra_bench.py [out.md] [--quick]

One process.  Per size every variant is warmed up once, then the variants are timed in turn, five rounds, each timing a
host clock around one synchronous call; the table has the median (min, max).  Before any time is kept the entropies of
all variants are compared at the tolerance of the tests (1e-10).  Sizes: the band-limit model (13 molecules, 4 phonon
levels) and a 25-molecule Holstein chain with 16 phonon levels, each at D = 8, 16, 32 and 64, normalised random complex
states from a fixed seed; and the spin-boson chain of examples/sbm.py (Ohmic bath, 300 modes) at D = 64 after two
TDVP-PS steps from the padded product state.  The largest number of Jacobi sweeps of a solve is printed at the end."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS = 5
TOL = 1e-10
ENV = "MPSE_BOND_SPECTRA_CHAIN"


def sizes(quick):
    if quick:
        return [("band limit", 5, 4, 8), ("Holstein", 4, 4, 16), ("spin-boson", 10, 0, 16)]
    return ([("band limit", 13, 4, D) for D in (8, 16, 32, 64)] + [("Holstein", 25, 16, D) for D in (8, 16, 32, 64)] +
            [("spin-boson", 300, 0, 64)])


def build(kind, nmol, pdim, D):
    from renormalizer_amd import (CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, HolsteinModel, Mol, Mpo,
                                  Phonon, Quantity)
    from renormalizer_amd.mps.mps import Mps
    if kind == "spin-boson":
        from renormalizer_amd.sbm import param2mollist
        model = param2mollist(alpha=0.05, raw_delta=Quantity(1), omega_c=Quantity(20), renormalization_p=1, n_phonons=nmol)
        mpo = Mpo(model)
        mps = Mps.ground_state(model, False)
        mps.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=D)
        mps.evolve_config = EvolveConfig(EvolveMethod.tdvp_ps)
        mps = mps.expand_bond_dimension(mpo, coef=1e-16, include_ex=False)
        for _ in range(2):
            mps = mps.evolve(mpo, 0.1)
        return mps
    if kind == "band limit":
        ph = Phonon.simple_phonon(Quantity(1e-10, "cm^{-1}"), Quantity(1e-10, "a.u."), pdim)
        model = HolsteinModel([Mol(Quantity(0), [ph])] * nmol, Quantity(0.8, "eV"), 3)
    else:
        ph = Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.274571056529368), pdim)
        model = HolsteinModel([Mol(Quantity(0), [ph])] * nmol, Quantity(3.0e-2), 3)
    mps = Mps.random(model, 1, D, rng=np.random.default_rng(nmol * 1000 + D)).to_complex()
    mps.canonicalise().normalize("mps_only")
    return mps


def timed(fn):
    t0 = time.perf_counter()
    val = fn()
    return time.perf_counter() - t0, val


def with_env(value, fn):
    def run():
        old = os.environ.pop(ENV, None)
        os.environ[ENV] = value
        try:
            return fn()
        finally:
            os.environ.pop(ENV, None)
            if old is not None:
                os.environ[ENV] = old
    return run


def main():
    from renormalizer_amd.engine import get_engine, mps_bond_spectra_plan
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    eng = get_engine()
    lines = [f"{ROUNDS} rounds, the variants in turn inside each round, one synchronous call per timing (host clock) after "
             "one warm-up call per variant; median (min, max) in ms.  All variants agree to 1e-10 in the entropies before "
             "a time is kept.", "",
             "| model | sites | largest bond | `calc_bond_entropy()` | `bond_entropies()`, chain kernels | "
             "`bond_entropies()`, enqueued | calc / enqueued | enqueued / chain | calc / chain |", "|" + "---|" * 9]
    for kind, nmol, pdim, D in sizes(quick):
        mps = build(kind, nmol, pdim, D)
        n = len(mps)
        chain_ok = mps_bond_spectra_plan(eng.corr_dims(mps._mp), n - 1, mps.is_complex)[1]["lds_fit_bytes"] > 0
        variants = {"old": mps.calc_bond_entropy, "enq": with_env("0", mps.bond_entropies)}
        if chain_ok:
            variants["chain"] = with_env("1", mps.bond_entropies)
        s0 = eng.mps_bond_spectra_stats()
        vals = {name: fn() for name, fn in variants.items()}          # warm-up, and the values
        s1 = eng.mps_bond_spectra_stats()
        assert s1["enqueued"] - s0["enqueued"] == 1 and s1["chain_kernel"] - s0["chain_kernel"] == int(chain_ok), (s0, s1)
        for name, v in vals.items():
            err = np.abs(v - vals["old"]).max()
            print(f"{kind} {nmol} x {pdim}, D = {max(mps.bond_dims)}: |{name} - old| = {err:.2e}", flush=True)
            assert err <= TOL, (name, err)
        times = {name: [] for name in variants}
        for _ in range(ROUNDS):
            for name, fn in variants.items():
                eng.sync()
                times[name].append(timed(fn)[0])

        def fmt(name):
            if name not in times:
                return "-"
            ts = np.array(times[name]) * 1e3
            return f"{np.median(ts):.2f} ({ts.min():.2f}, {ts.max():.2f})"

        def ratio(a, b):
            if a not in times or b not in times:
                return "-"
            return f"{np.median(times[a]) / np.median(times[b]):.1f}"

        label = kind if kind == "spin-boson" else f"{kind}, {nmol} molecules, {pdim} levels"
        lines.append(f"| {label} | {n} | {max(mps.bond_dims)} | {fmt('old')} | {fmt('chain')} | {fmt('enq')} | "
                     f"{ratio('old', 'enq')} | {ratio('enq', 'chain')} | {ratio('old', 'chain')} |")
        print(lines[-1], flush=True)
    lines += ["", f"Largest number of Jacobi sweeps of one solve over these calls: "
              f"{eng.mps_bond_spectra_stats()['max_sweeps']}."]
    text = "\n".join(lines) + "\n"
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
