#!/usr/bin/env python3
"""Times the electron's reduced density matrix rho_ij = <a_i^+ a_j> three ways on one GPU: ``Mps.calc_edof_rdm()`` (one
MPO window per entry through ``expectations``, the path ``Mps.edof_rdm()`` replaces), ``Mps.edof_rdm()`` through the
chain kernels of ``mpse_mps_corr`` (MPSE_CORR_CHAIN=1: every chain whose launches fit, also above the bond limit of the
path rule, which is read off this table) and through its enqueued products (MPSE_CORR_CHAIN=0).

    python tools/corr_bench.py [out.md] [--quick]

One process.  Per size every variant is warmed up once, then the variants are timed in turn, three rounds, each timing a
host clock around one synchronous call.  Before any time is kept the results of all variants are compared at the
tolerance of the tests (1e-12 on a normalised state).  Sizes: the band-limit model (13 molecules, 4 phonon levels) at
D = 16 and 32, and a 25-molecule Holstein chain with 16 phonon levels at D = 64 (the chain kernels' limit), 128 and 256
(enqueued products only); normalised random complex states from a fixed seed."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS = 3
TOL = 1e-12


def sizes(quick):
    if quick:
        return [("band limit", 5, 4, 8), ("Holstein", 4, 4, 16)]
    return [("band limit", 13, 4, 16), ("band limit", 13, 4, 32), ("Holstein", 25, 16, 64), ("Holstein", 25, 16, 128),
            ("Holstein", 25, 16, 256)]


def build(kind, nmol, pdim, D):
    from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity
    from renormalizer_amd.mps.mps import Mps
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
        old = os.environ.pop("MPSE_CORR_CHAIN", None)
        if value is not None:
            os.environ["MPSE_CORR_CHAIN"] = value
        try:
            return fn()
        finally:
            os.environ.pop("MPSE_CORR_CHAIN", None)
            if old is not None:
                os.environ["MPSE_CORR_CHAIN"] = old
    return run


def main():
    from renormalizer_amd.engine import get_engine, mps_corr_plan
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    eng = get_engine()
    lines = [f"{ROUNDS} rounds, the variants in turn inside each round, one synchronous call per timing (host clock) after "
             "one warm-up call per variant; median (min, max).  All variants agree to 1e-12 before a time is kept.", "",
             "| model | molecules | phonon levels | largest bond | `calc_edof_rdm()` | `edof_rdm()`, chain kernels | "
             "`edof_rdm()`, enqueued products | calc / chain | calc / enqueued | enqueued / chain |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for kind, nmol, pdim, D in sizes(quick):
        mps = build(kind, nmol, pdim, D)
        sel = [mps.model.dof_to_siteidx[d] for d in mps.model.e_dofs]
        chain_ok = mps_corr_plan(eng.corr_dims(mps._mp), len(sel), True)[1]["lds_fit_bytes"] > 0
        variants = {"calc": mps.calc_edof_rdm, "enqueued": with_env("0", mps.edof_rdm)}
        if chain_ok:
            variants["chain"] = with_env("1", mps.edof_rdm)
        s0 = eng.mps_corr_stats()
        vals = {name: fn() for name, fn in variants.items()}          # warm-up, and the values
        s1 = eng.mps_corr_stats()
        assert s1["enqueued"] - s0["enqueued"] == 1 and s1["chain_kernel"] - s0["chain_kernel"] == int(chain_ok), (s0, s1)
        for name, v in vals.items():
            err = np.abs(v - vals["calc"]).max()
            print(f"{kind} {nmol} x {pdim}, D = {max(mps.bond_dims)}: |{name} - calc| = {err:.2e}", flush=True)
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
            return f"{np.median(ts):.2f} ms ({ts.min():.2f}, {ts.max():.2f})"

        def ratio(a, b):
            if a not in times or b not in times:
                return "-"
            return f"{np.median(times[a]) / np.median(times[b]):.1f}"

        lines.append(f"| {kind} | {nmol} | {pdim} | {max(mps.bond_dims)} | {fmt('calc')} | {fmt('chain')} | {fmt('enqueued')} | "
                     f"{ratio('calc', 'chain')} | {ratio('calc', 'enqueued')} | {ratio('enqueued', 'chain')} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
