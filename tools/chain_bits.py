#!/usr/bin/env python3
"""Prints one sha256 of the raw result bytes per case of the six chain calls with a selection (``Engine.mps_corr``,
``mps_rdm1``, ``mps_rdm2``, ``mps_trdm1``, ``mps_bond_spectra``, ``mps_expect_many``), each on both paths (MPSE_*_CHAIN=1
and =0), for a fixed list of seeded inputs, on one GPU.

    python tools/chain_bits.py [out.txt]

Two libraries of one ABI compute the same bits when their outputs are the same text: run it once per library
(RENO_MPSENGINE selects one) on the same machine and compare.  The order of every sum in these calls is fixed, so a
line depends on the inputs and the code alone.  The cases are small, a call takes milliseconds: chains of 3 to 6 sites
with bonds that are no power of two, two chains with different bonds, d of 1, 2, 5 and 17 (one more than the waves of a
workgroup), an ancilla leg of 1 and 2, three sites of d = 2 at bond 64 (the full LDS plan) and 64 against 1, real,
complex and mixed sites, full selections and selections that start after site 0 and end before the last site."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MIXED = (False, True, True, False, True, False)

# (name, bonds, d per site, ancilla extent or None, complex flag(s), selection of sites)
CHAINS = [
    ("b12321 d2 real full", (1, 2, 3, 2, 1), (2, 2, 2, 2), None, False, (0, 1, 2, 3)),
    ("b12321 d2 cplx full", (1, 2, 3, 2, 1), (2, 2, 2, 2), None, True, (0, 1, 2, 3)),
    ("b12321 d2 mixed inner", (1, 2, 3, 2, 1), (2, 2, 2, 2), None, MIXED[:4], (1, 2)),
    ("b1253421 d5 danc2 cplx inner", (1, 2, 5, 3, 4, 2, 1), (5, 2, 5, 1, 5, 2), 2, True, (1, 3, 4)),
    ("b1253421 d5 danc2 real full", (1, 2, 5, 3, 4, 2, 1), (5, 2, 5, 1, 5, 2), 2, False, (0, 1, 2, 3, 4, 5)),
    ("b1253421 d5 danc1 mixed inner", (1, 2, 5, 3, 4, 2, 1), (5, 2, 5, 1, 5, 2), 1, MIXED, (1, 2, 4)),
    ("b13431 d17 cplx full", (1, 3, 4, 3, 1), (17, 2, 17, 1), None, True, (0, 1, 2, 3)),
    ("b13431 d17 real inner", (1, 3, 4, 3, 1), (17, 2, 17, 1), None, False, (1, 2)),
    ("b1 64 64 1 d2 cplx full", (1, 64, 64, 1), (2, 2, 2), None, True, (0, 1, 2)),
    ("b1 64 64 1 d2 real full", (1, 64, 64, 1), (2, 2, 2), None, False, (0, 1, 2)),
]
# the bra of the two-chain cases: other bonds on the same sites; None: the bonds of the ket
BRA_BONDS = {(1, 2, 3, 2, 1): (1, 3, 2, 4, 1), (1, 2, 5, 3, 4, 2, 1): (1, 3, 7, 10, 5, 2, 1), (1, 3, 4, 3, 1): (1, 1, 1, 1, 1),
             (1, 64, 64, 1): (1, 1, 1, 1)}
SWITCH = {"corr": "MPSE_CORR_CHAIN", "rdm1": "MPSE_RDM1_CHAIN", "rdm2": "MPSE_RDM2_CHAIN", "trdm1": "MPSE_TRDM1_CHAIN",
          "bond_spectra": "MPSE_BOND_SPECTRA_CHAIN", "expect_many": "MPSE_EXPECT_CHAIN"}


def rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def chain(rng, bonds, ds, danc, cplx):
    fl = [cplx] * len(ds) if isinstance(cplx, bool) else list(cplx)
    return [rand(rng, (bonds[i], d) + (() if danc is None else (danc,)) + (bonds[i + 1],), fl[i]) / np.sqrt(bonds[i] * d)
            for i, d in enumerate(ds)]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    from renormalizer_amd.engine import get_engine
    eng = get_engine()
    lines = []

    def dev(arrays):
        return [eng.asdevice(np.ascontiguousarray(a)) for a in arrays]

    def both(call, label, fn, stats):
        for env in ("1", "0"):
            os.environ[SWITCH[call]] = env
            s0 = stats()
            out = fn()
            s1 = stats()
            # =1 takes the kernels wherever the launches fit (expect_many at bond 64 does not: the line says so)
            took = "chain" if s1["chain_kernel"] > s0["chain_kernel"] else "enqueued"
            assert env == "1" or took == "enqueued", (call, label, s0, s1)
            lines.append(f"{call:13s} {took:8s} {label:44s} {digest(out)}")
            print(lines[-1], flush=True)
        del os.environ[SWITCH[call]]

    for seed, (name, bonds, ds, danc, cplx, sel) in enumerate(CHAINS):
        rng = np.random.default_rng(1000 + seed)
        n = len(ds)
        ket = chain(rng, bonds, ds, danc, cplx)
        dket = dev(ket)
        mats = [[rand(rng, (ds[k], ds[k]), True) for k in sel] for _ in range(3)]
        both("corr", name, lambda: [eng.mps_corr(dket, sel, *mats)], eng.mps_corr_stats)
        both("rdm1", name, lambda: eng.mps_rdm1(dket, sel), eng.mps_rdm1_stats)
        both("rdm2", name, lambda: list(eng.mps_rdm2(dket, sel).values()), eng.mps_rdm2_stats)
        # bonds: the selected sites but the last name the bonds right of them; and the first and the last bond alone
        for bsel in (tuple(k for k in sel if k < n - 1), (0, n - 2)):
            both("bond_spectra", f"{name} bonds {bsel}", lambda: eng.mps_bond_spectra(dket, bsel),
                 eng.mps_bond_spectra_stats)
        # operators: one MPO site of bond 1 on every selected site, and a window of MPO bond 2 from the first to the last
        ops = [(k, dev([rand(rng, (1, ds[k], ds[k], 1), True)])) for k in sel]
        first, last = sel[0], sel[-1]
        if last > first:
            wb = [1] + [2] * (last - first) + [1]
            ops.append((first, dev([rand(rng, (wb[j], ds[first + j], ds[first + j], wb[j + 1]), bool(j % 2))
                                    for j in range(last - first + 1)])))
        both("expect_many", name, lambda: [eng.mps_expect_many(dket, ops)], eng.mps_expect_many_stats)
        # two chains: a bra of other bonds, real where the ket is complex at the odd sites; and the ket as its own bra
        fl = [cplx] * n if isinstance(cplx, bool) else list(cplx)
        bra = chain(rng, BRA_BONDS[bonds], ds, danc, [f != bool(i % 2) for i, f in enumerate(fl)])
        dbra = dev(bra)
        for conj in (True, False):
            both("trdm1", f"{name} conj={int(conj)}", lambda: eng.mps_trdm1(dbra, dket, sel, conj), eng.mps_trdm1_stats)
        both("trdm1", f"{name} swapped", lambda: eng.mps_trdm1(dket, dbra, sel, True), eng.mps_trdm1_stats)
        both("trdm1", f"{name} bra=ket", lambda: eng.mps_trdm1(dket, dket, sel, True), eng.mps_trdm1_stats)
    text = "\n".join(lines) + "\n"
    print("sha256 of all lines:", hashlib.sha256(text.encode()).hexdigest())
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
