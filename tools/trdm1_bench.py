#!/usr/bin/env python3
"""Times the row of transition matrix elements <bra| O_i |ket> taken after every step of a Green's function, on one GPU:
as ``ket.expectations(opers, bra.conj())`` (a conjugated copy of the bra, then one operator window, one closing product
and one host read per degree of freedom) and as ``bra.transition_elements(symbol, dofs, ket, self_is_conj=False)`` (one
engine call, ``mpse_mps_trdm1``) through the chain kernels (MPSE_TRDM1_CHAIN=1: every pair of chains whose launches fit,
also above the bond limits of the path rule, which are read off this table) and through the enqueued products
(MPSE_TRDM1_CHAIN=0).

    python tools/trdm1_bench.py [out.md] [--quick]

One process.  Per size every variant is warmed up once, then the variants are timed in turn, five rounds, each timing a
host clock around one synchronous call.  Before any time is kept the results of all variants are compared at the
tolerance of the tests (1e-12 on normalised states).  Sizes: a product-state bra (the ground state, every bond 1, O = a)
against a ket of bond 16, 32, 64 and 256, and a bra of the ket's bonds (the ket with every element turned by a small
random phase, O = a^+ a) at 8, 16 and 32; each on the band-limit model (13 molecules, 4 phonon levels: d = 2 / 4) and on
a 25-molecule Holstein chain with 16 phonon levels (d = 2 / 16); normalised random complex states from a fixed seed."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS = 5
TOL = 1e-12
ENV = "MPSE_TRDM1_CHAIN"


def sizes(quick):
    if quick:
        return [("band limit", 5, 4, 1, 8), ("Holstein", 4, 4, 8, 8)]
    models = (("band limit", 13, 4), ("Holstein", 25, 16))
    return [m + (1, D) for m in models for D in (16, 32, 64, 256)] + [m + (D, D) for m in models for D in (8, 16, 32)]


def build(kind, nmol, pdim, Db, Dk):
    """(bra, ket, symbol): Db = 1: the ground state as bra and O = a; else a bra of the ket's bonds and O = a^+ a"""
    from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity
    from renormalizer_amd.mps.mps import Mps
    if kind == "band limit":
        ph = Phonon.simple_phonon(Quantity(1e-10, "cm^{-1}"), Quantity(1e-10, "a.u."), pdim)
        model = HolsteinModel([Mol(Quantity(0), [ph])] * nmol, Quantity(0.8, "eV"), 3)
    else:
        ph = Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.274571056529368), pdim)
        model = HolsteinModel([Mol(Quantity(0), [ph])] * nmol, Quantity(3.0e-2), 3)

    def rand(D, seed):
        mps = Mps.random(model, 1, D, rng=np.random.default_rng(seed)).to_complex()
        mps.canonicalise().normalize("mps_only")
        return mps

    ket = rand(Dk, nmol * 1000 + Dk)
    if Db == 1:
        return Mps.ground_state(model, False), ket, "a"
    # a bra of the ket's bonds that is another state but overlaps with it (two independent random states of 50 sites
    # have matrix elements of 1e-16, which would compare zeros): every element of the ket turned by a small random phase
    bra = ket.copy()
    for i in range(len(bra)):
        a = bra[i].to_host()
        bra[i] = a * np.exp(0.1j * np.random.default_rng(nmol * 1000 + Db + 7 + i).uniform(-1, 1, a.shape))
    bra.canonicalise().normalize("mps_only")
    return bra, ket, r"a^\dagger a"


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
    from renormalizer_amd import Mpo, Op
    from renormalizer_amd.engine import get_engine, mps_trdm1_plan
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    eng = get_engine()
    lines = [f"{ROUNDS} rounds, the variants in turn inside each round, one synchronous call per timing (host clock) after "
             "one warm-up call per variant; median (min, max) in ms.  All variants agree to 1e-12 before a time is kept.",
             "", "| model | molecules | phonon levels | sites | operators | bra bond | ket bond | "
             "`expectations(opers, bra.conj())` | `transition_elements`, chain kernels | `transition_elements`, enqueued "
             "| old / enqueued | enqueued / chain | old / chain |", "|" + "---|" * 13]
    for kind, nmol, pdim, Db, Dk in sizes(quick):
        bra, ket, sym = build(kind, nmol, pdim, Db, Dk)
        model = ket.model
        n, dofs = len(ket), list(model.e_dofs)
        opers = [Mpo(model, Op(sym, dof)) for dof in dofs]
        fits = mps_trdm1_plan(eng.trdm1_dims(bra._mp, ket._mp), len(dofs), True)[1]["lds_fit_bytes"] > 0

        def old():
            return np.asarray(ket.expectations(opers, bra.conj()), dtype=np.complex128)

        def new():
            return bra.transition_elements(sym, dofs, ket, self_is_conj=False)

        variants = {"old": old, "enq": with_env("0", new)}
        if fits:
            variants["chain"] = with_env("1", new)
        s0 = eng.mps_trdm1_stats()
        vals = {name: fn() for name, fn in variants.items()}          # warm-up, and the values
        s1 = eng.mps_trdm1_stats()
        assert s1["enqueued"] - s0["enqueued"] == 1 and s1["chain_kernel"] - s0["chain_kernel"] == int(fits), (s0, s1)
        for name, v in vals.items():
            # ``expectation`` returns the real part alone when the imaginary part is zero to ``np.isclose`` (below
            # 1e-8): the new values meet the old ones after the same rule
            if name != "old":
                v = np.where(np.isclose(v.imag, 0), v.real, v)
            err = np.abs(v - vals["old"]).max()
            print(f"{kind} {nmol} x {pdim}, bonds {max(bra.bond_dims)} / {max(ket.bond_dims)}: |{name} - old| = {err:.2e}, "
                  f"largest value {np.abs(vals['old']).max():.2e}", flush=True)
            assert err <= TOL, (name, err)
        if fits:
            assert np.abs(vals["chain"] - vals["enq"]).max() <= TOL          # the two paths, imaginary parts included
        times ={name: [] for name in variants}
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

        lines.append(f"| {kind} | {nmol} | {pdim} | {n} | {len(dofs)} | {max(bra.bond_dims)} | {max(ket.bond_dims)} | "
                     f"{fmt('old')} | {fmt('chain')} | {fmt('enq')} | {ratio('old', 'enq')} | {ratio('enq', 'chain')} | "
                     f"{ratio('old', 'chain')} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
