#!/usr/bin/env python3
"""Times the local observables taken after every step, on one GPU: the one-site reduced density matrices of all sites
as ``Mps.calc_1site_rdm()`` (three products and a host read per site) and as ``Mps.site_rdms()`` (one engine call,
``mpse_mps_rdm1``), and the occupations as ``Mps.e_occupations`` + ``Mps.ph_occupations`` (one operator window and one
host read per degree of freedom) and as ``Mps.occupations()`` (one engine call).  The one-call variants run through the
chain kernels (MPSE_RDM1_CHAIN=1: every chain whose launches fit, also above the bond limit of the path rule, which is
read off this table) and through the enqueued products (MPSE_RDM1_CHAIN=0).

    python tools/rdm1_bench.py [out.md] [--quick]

One process.  Per size every variant is warmed up once, then the variants are timed in turn, three rounds, each timing a
host clock around one synchronous call.  Before any time is kept the results of all variants are compared at the
tolerance of the tests (1e-12 on a normalised state).  Sizes: the band-limit model (13 molecules, 4 phonon levels) at
D = 8, 16 and 32, and a 25-molecule Holstein chain with 16 phonon levels at D = 16, 32, 64 (the chain kernels' limit),
128 and 256 (enqueued products only); normalised random complex states from a fixed seed."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS = 3
TOL = 1e-12
ENV = "MPSE_RDM1_CHAIN"


def sizes(quick):
    if quick:
        return [("band limit", 5, 4, 8), ("Holstein", 4, 4, 16)]
    return [("band limit", 13, 4, 8), ("band limit", 13, 4, 16), ("band limit", 13, 4, 32), ("Holstein", 25, 16, 16),
            ("Holstein", 25, 16, 32), ("Holstein", 25, 16, 64), ("Holstein", 25, 16, 128), ("Holstein", 25, 16, 256)]


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
    from renormalizer_amd.engine import get_engine, mps_rdm1_plan
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    eng = get_engine()
    lines = [f"{ROUNDS} rounds, the variants in turn inside each round, one synchronous call per timing (host clock) after "
             "one warm-up call per variant; median (min, max) in ms.  All variants agree to 1e-12 before a time is kept.",
             "", "| model | molecules | phonon levels | sites | largest bond | `calc_1site_rdm()` | `site_rdms()`, chain "
             "kernels | `site_rdms()`, enqueued | `e_occupations` + `ph_occupations` | `occupations()`, chain kernels | "
             "`occupations()`, enqueued | rdm: calc / enqueued | rdm: enqueued / chain | occ: old / enqueued | occ: "
             "enqueued / chain |", "|" + "---|" * 15]
    for kind, nmol, pdim, D in sizes(quick):
        mps = build(kind, nmol, pdim, D)
        n = len(mps)
        chain_ok = mps_rdm1_plan(eng.corr_dims(mps._mp), n, True)[1]["lds_fit_bytes"] > 0

        def rdm_old():
            return mps.calc_1site_rdm()

        def occ_old():
            return np.asarray(mps.e_occupations), np.asarray(mps.ph_occupations)

        variants = {"rdm_old": rdm_old, "rdm_enq": with_env("0", mps.site_rdms), "occ_old": occ_old,
                    "occ_enq": with_env("0", mps.occupations)}
        if chain_ok:
            variants["rdm_chain"] = with_env("1", mps.site_rdms)
            variants["occ_chain"] = with_env("1", mps.occupations)
        s0 = eng.mps_rdm1_stats()
        vals = {name: fn() for name, fn in variants.items()}          # warm-up, and the values
        s1 = eng.mps_rdm1_stats()
        assert s1["enqueued"] - s0["enqueued"] == 2 and s1["chain_kernel"] - s0["chain_kernel"] == 2 * int(chain_ok), (s0, s1)
        for name, v in vals.items():
            if name.startswith("rdm"):
                err = max(np.abs(v[k] - vals["rdm_old"][k]).max() for k in range(n))
            else:
                err = max(np.abs(a - b).max() for a, b in zip(v, vals["occ_old"]))
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

        lines.append(f"| {kind} | {nmol} | {pdim} | {n} | {max(mps.bond_dims)} | {fmt('rdm_old')} | {fmt('rdm_chain')} | "
                     f"{fmt('rdm_enq')} | {fmt('occ_old')} | {fmt('occ_chain')} | {fmt('occ_enq')} | "
                     f"{ratio('rdm_old', 'rdm_enq')} | {ratio('rdm_enq', 'rdm_chain')} | {ratio('occ_old', 'occ_enq')} | "
                     f"{ratio('occ_enq', 'occ_chain')} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
