#!/usr/bin/env python3
"""Times the two-site reduced density matrices of all pairs of a selection of sites, on one GPU: the parent's path
(``Mps.calc_2site_rdm()``: strided products pushed one site at a time per pair, a host read per pair) and
``Mps.pair_rdms()`` (one engine call, ``mpse_mps_rdm2``) through the chain kernels (MPSE_RDM2_CHAIN=1: every chain whose
launches fit, also above the bond limit of the path rule, which is read off this table) and through the enqueued
products (MPSE_RDM2_CHAIN=0).

    python tools/rdm2_bench.py [out.md] [--quick]

One process.  Per size every variant is warmed up once, then the variants are timed in turn, three rounds, each timing a
host clock around one synchronous call.  Before any time is kept the results of all variants are compared at the
tolerance of the tests (1e-12 on a normalised state).  Sizes: the band-limit model (13 molecules, 4 phonon levels, all
26 sites selected) at D = 8, 16 and 32, and a 25-molecule Holstein chain with 16 phonon levels, whose selection is the
25 electronic sites plus the 4 phonon sites at the centre so that the result stays small, at D = 16, 32, 64 (the chain
kernels' limit), 128 and 256 (enqueued products only); normalised random complex states from a fixed seed.

``calc_2site_rdm()`` has no selection: where not every site is selected the parent's path is ``calc_pairs`` below, its
loop with the sites that open and close restricted to the selection (checked against ``calc_2site_rdm()`` itself, byte
for byte, on the first size of the run where that is affordable)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS = 3
TOL = 1e-12
ENV = "MPSE_RDM2_CHAIN"


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


def selection(kind, mps):
    """all sites of the band-limit chain; the electronic sites plus the 4 phonon sites nearest the centre otherwise"""
    n = len(mps)
    if kind == "band limit":
        return list(range(n))
    e_sites = sorted({mps.model.dof_to_siteidx[d] for d in mps.model.e_dofs})
    v_sites = sorted({mps.model.dof_to_siteidx[d] for d in mps.model.v_dofs}, key=lambda s: (abs(s - n / 2), s))
    return sorted(set(e_sites) | set(v_sites[:4]))


def calc_pairs(mps, sel):
    """the loop of ``Mps.calc_2site_rdm`` (renormalizer_amd/mps/mps.py) with opening and closing sites restricted to
    ``sel``: the same products in the same order for the pairs it keeps, a host read per pair"""
    from renormalizer_amd.engine import get_engine, idx1, idx2
    from renormalizer_amd.mps.mps import contract_one_site
    eng = get_engine()
    n = mps.site_num
    ident = [eng.asdevice(np.eye(mps[i].shape[1]).reshape(1, mps[i].shape[1], mps[i].shape[1], 1)) for i in range(n)]
    sentinel = eng.ones((1, 1, 1), np.float64)
    sentinel.unit = 1
    lenv = {-1: sentinel}
    for i in range(n - 1):
        lenv[i] = contract_one_site(lenv[i - 1], mps[i], ident[i], "L")
    renv = {n: sentinel}
    for i in range(n - 1, 0, -1):
        renv[i] = contract_one_site(renv[i + 1], mps[i], ident[i], "R")

    def shape(a):
        Dl, d, Dr = a.shape[0], a.shape[1], a.shape[-1]
        return Dl, d, a.size // (Dl * d * Dr), Dr

    def left_component(i):
        a = mps[i]
        Dl, d, da, Dr = shape(a)
        x = eng.matmul(lenv[i - 1].reshape(Dl, Dl), a.reshape(Dl, d * da * Dr), trans_a=True, conj_b=True)
        t = eng.empty((d * d, Dr * Dr), np.complex128 if (x.is_complex or a.is_complex) else np.float64)
        a2, x2 = (a.to_complex(), x.to_complex()) if t.is_complex else (a, x)
        eng.gemm(x2, a2, t, idx2(d, Dr, da * Dr, 1), idx2(Dl, da, d * da * Dr, Dr), idx2(Dl, da, d * da * Dr, Dr),
                 idx2(d, Dr, da * Dr, 1), idx2(d, Dr, d * Dr * Dr, Dr), idx2(d, Dr, Dr * Dr, 1))
        return t

    def right_component(j):
        a = mps[j]
        Dl, d, da, Dr = shape(a)
        y = eng.matmul(a.reshape(Dl * d * da, Dr), renv[j + 1].reshape(Dr, Dr), conj_a=True)
        rc = eng.empty((Dl * Dl, d * d), np.complex128 if (y.is_complex or a.is_complex) else np.float64)
        a2, y2 = (a.to_complex(), y.to_complex()) if rc.is_complex else (a, y)
        eng.gemm(y2, a2, rc, idx1(Dl * d, da * Dr), idx1(da * Dr, 1), idx1(da * Dr, 1), idx1(Dl * d, da * Dr),
                 idx2(Dl, d, Dl * d * d, d), idx2(Dl, d, d * d, 1))
        return rc

    def transfer(t, k, dd):
        a = mps[k]
        D, Dc = a.shape[0], a.shape[-1]
        dk = a.size // (D * Dc)
        cdt = np.complex128 if (t.is_complex or a.is_complex) else np.float64
        a2, t2 = (a.to_complex(), t.to_complex()) if cdt == np.complex128 else (a, t)
        u = eng.empty((dd * D, dk * Dc), cdt)
        eng.gemm(t2, a2, u, idx2(dd, D, D * D, 1), idx1(D, D), idx1(D, dk * Dc), idx1(dk * Dc, 1),
                 idx1(dd * D, dk * Dc), idx1(dk * Dc, 1), conj_b=True)
        out = eng.empty((dd, Dc * Dc), cdt)
        eng.gemm(u, a2, out, idx2(dd, Dc, D * dk * Dc, 1), idx1(D * dk, Dc), idx1(D * dk, Dc), idx1(Dc, 1),
                 idx2(dd, Dc, Dc * Dc, Dc), idx1(Dc, 1))
        return out

    rcs = {j: right_component(j) for j in sel[1:]}
    rdm = {}
    for i in sel[:-1]:
        di = mps[i].shape[1]
        t = left_component(i)
        for j in range(i + 1, sel[-1] + 1):
            if j != i + 1:
                t = transfer(t, j - 1, di * di)
            if j in rcs:
                dj = mps[j].shape[1]
                res = eng.matmul(t, rcs[j]).to_host().reshape(di, di, dj, dj)
                rdm[(i, j)] = res.transpose(0, 2, 1, 3).reshape(di * dj, di * dj)
    return rdm


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
    from renormalizer_amd.engine import get_engine, mps_rdm2_plan
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    eng = get_engine()
    lines = [f"{ROUNDS} rounds, the variants in turn inside each round, one synchronous call per timing (host clock) after "
             "one warm-up call per variant; median (min, max) in ms.  All variants agree to 1e-12 before a time is kept.",
             "", "| model | molecules | phonon levels | sites | selected | pairs | largest bond | `calc_2site_rdm()` | "
             "`pair_rdms()`, chain kernels | `pair_rdms()`, enqueued | calc / enqueued | enqueued / chain |",
             "|" + "---|" * 12]
    checked_old = False
    for kind, nmol, pdim, D in sizes(quick):
        mps = build(kind, nmol, pdim, D)
        n = len(mps)
        sel = selection(kind, mps)
        npair = len(sel) * (len(sel) - 1) // 2
        chain_ok = mps_rdm2_plan(eng.corr_dims(mps._mp), sel, True)[1]["lds_fit_bytes"] > 0
        if len(sel) == n:
            old = mps.calc_2site_rdm
            if not checked_old:      # the restricted loop is the parent's loop: the same bytes where both are defined
                a, b = mps.calc_2site_rdm(), calc_pairs(mps, sel)
                assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
                checked_old = True
        else:
            def old():
                return calc_pairs(mps, sel)

        def new():
            return mps.pair_rdms(sel)

        variants = {"old": old, "enq": with_env("0", new)}
        if chain_ok:
            variants["chain"] = with_env("1", new)
        s0 = eng.mps_rdm2_stats()
        vals = {name: fn() for name, fn in variants.items()}          # warm-up, and the values
        s1 = eng.mps_rdm2_stats()
        assert s1["enqueued"] - s0["enqueued"] == 1 and s1["chain_kernel"] - s0["chain_kernel"] == int(chain_ok), (s0, s1)
        for name, v in vals.items():
            assert len(v) == npair and sorted(v) == sorted(vals["old"])
            err = max(np.abs(v[k] - vals["old"][k]).max() for k in v)
            print(f"{kind} {nmol} x {pdim}, D = {max(mps.bond_dims)}: |{name} - old| = {err:.2e}", flush=True)
            assert err <= TOL, (name, err)
        del vals
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

        lines.append(f"| {kind} | {nmol} | {pdim} | {n} | {len(sel)} | {npair} | {max(mps.bond_dims)} | {fmt('old')} | "
                     f"{fmt('chain')} | {fmt('enq')} | {ratio('old', 'enq')} | {ratio('enq', 'chain')} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
