#!/usr/bin/env python3
"""Times the centre solve of the finite-temperature correction vector (mpse_pcg_sum over M1 + 2 M2 + M3) on synthetic
one-site centres (D, d, d, D) with MPO bonds of 5, against the same system on the code path that needs none of the new
engine entry points: the combined operator (a (x) 1 + 1 (x) H^T) as ONE MPO (bond 5 + 5, the direct sum ``Mpo.add``
gives) on a single physical leg of size d^2, squared by mpse_heff_apply2 inside mpse_pcg.  Both run a fixed number of
iterations (tol = 0).  Per size: time per iteration of either form, the three term applications timed one by one
(mpse_heff_apply_ft between two synchronisations) and what is left for the vector kernels.  Then the wall time of
``SpectraFtCV.cv_solve`` per frequency for the reference's absorption test.  Prints markdown.  Not part of bench.py.

    python tools/cv_ft_probe.py [--sizes 10x4 64x4 64x16] [--iters 24] [--repeats 5] [--no-spectrum]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity  # noqa: E402
from renormalizer_amd.engine import LEG_DOWN, LEG_UP, get_engine  # noqa: E402
from renormalizer_amd.mps.hop_expr import hop_expr  # noqa: E402
from renormalizer_amd.utils import constant  # noqa: E402

W = 5


def sym(rng, n, scale):
    a = rng.standard_normal((n, n)) * scale / np.sqrt(n)
    return (a + a.T) / 2


def one_layer(D, d, fl, fs, fr):
    """(L, W, R) of fl (x) 1 (x) 1 + 1 (x) fs (x) 1 + 1 (x) 1 (x) fr with two idle channels (bond 5, like a Holstein MPO)"""
    l, r, w = np.zeros((D, W, D)), np.zeros((D, W, D)), np.zeros((W, d, d, W))
    for ch in range(W):
        l[:, ch, :] = fl if ch == 0 else np.eye(D)
        r[:, ch, :] = fr if ch == 2 else np.eye(D)
        if ch < 3:
            w[ch, :, :, ch] = fs if ch == 1 else np.eye(d)
    return l, w, r


def sq(e1, e2):
    return np.einsum("xba,dcx->abcd", e1, e2)


def timed(eng, fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def probe_size(eng, D, d, iters, repeats):
    rng = np.random.default_rng(3)
    fl, fu, fv, fr = sym(rng, D, 1.0), sym(rng, d, 1.0), sym(rng, d, 1.0), sym(rng, D, 1.0)
    la, wa, ra = one_layer(D, d, 0.6 * fl, fu, 0.3 * fr)
    lb, wb, rb = one_layer(D, d, 0.4 * fl, fv, 0.7 * fr)
    dev = eng.asdevice
    dwa, dwb = dev(wa), dev(wb)
    shape = (D, d, d, D)
    keep, terms = [], []
    for (l1, r1, w1, g1), (l2, r2, w2, g2) in (((la, ra, dwa, LEG_UP), (la, ra, dwa, LEG_UP)),
                                               ((la, ra, dwa, LEG_UP), (lb, rb, dwb, LEG_DOWN)),
                                               ((lb, rb, dwb, LEG_DOWN), (lb, rb, dwb, LEG_DOWN))):
        L, R = dev(sq(l1, l2)), dev(sq(r1, r2))
        keep += [L, R]
        terms.append(eng.ft_term(w1, w2, g1, g2, 0, 1, shape, L, R))
    b = dev(rng.standard_normal(shape))
    x0 = dev(rng.standard_normal(shape))
    factors = [eng.site_factor_ft(t) for t in terms]
    diag = eng.diag_ft_sum(terms, factors, (1.0, 2.0, 1.0), 0.25)
    # the baseline: one MPO on the leg of size d^2, channels of a and of H side by side
    wc = np.zeros((2 * W, d * d, d * d, 2 * W))
    wc[:W, :, :, :W] = np.einsum("bxyf,vw->bxvywf", wa, np.eye(d)).reshape(W, d * d, d * d, W)
    wc[W:, :, :, W:] = np.einsum("bxyf,uw->buxwyf", wb, np.eye(d)).reshape(W, d * d, d * d, W)
    # direct sum of the bonds: the operator is L_a W_a R_a + L_b W_b R_b = A + B, squared by the two layers
    lc, rc = np.concatenate([la, lb], axis=1), np.concatenate([ra, rb], axis=1)
    hop = hop_expr(dev(sq(lc, lc)), dev(sq(rc, rc)), [dev(wc)], (D, d * d, D), twolayer=True)
    bc, dc = b.reshape(D, d * d, D), diag.reshape(D, d * d, D)

    def run_sum():
        return eng.pcg_sum(terms, (1.0, 2.0, 1.0), b, x0.copy(), diag=diag, shift=0.25, tol=0.0, max_iter=iters,
                           check=False)

    def run_base():
        return eng.pcg(hop, bc, x0.copy().reshape(D, d * d, D), diag=dc, shift=0.25, tol=0.0, max_iter=iters, check=False)

    r1, r2 = run_sum(), run_base()
    t_sum, t_base = timed(eng, run_sum, repeats), timed(eng, run_base, repeats)
    apply_t = []
    for t in terms:
        apply_t.append(timed(eng, lambda t=t: [eng.heff_apply_ft(t, x0) for _ in range(iters)], repeats)[0] / iters)
    per_sum, per_base = t_sum[0] / max(r1.iters, 1), t_base[0] / max(r2.iters, 1)
    return dict(D=D, d=d, n=D * d * d * D, iters=(r1.iters, r2.iters), status=(r1.status, r2.status), per_sum=per_sum,
                spread_sum=(t_sum[1] / max(r1.iters, 1), t_sum[2] / max(r1.iters, 1)), per_base=per_base,
                spread_base=(t_base[1] / max(r2.iters, 1), t_base[2] / max(r2.iters, 1)), applies=apply_t)


def spectrum_times():
    from renormalizer_amd.cv import SpectraFtCV
    omega = [Quantity(106.51, "cm^{-1}"), Quantity(1555.55, "cm^{-1}")]
    dis = [Quantity(30.1370), Quantity(8.7729)]
    ph_list = [Phonon.simple_phonon(o, d, 4) for o, d in zip(omega, dis)]
    j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
    model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list, 15.45)] * 3, j)
    eng = get_engine()
    t0 = time.perf_counter()
    obj = SpectraFtCV(model, "abs", 10, 5.e-3, Quantity(298, "K"), Mpo(model, offset=Quantity(model.gs_zpe)), rtol=1e-3)
    print(f"\n### cv_solve per frequency, absorption test of the reference (m_max = 10); set-up {time.perf_counter() - t0:.2f} s\n")
    print("| omega | value | wall s | centre solves | CG iterations | host waits |")
    print("|---|---|---|---|---|---|")
    obj.batch_run = False
    for w in np.arange(0.08, 0.10, 2.e-3)[[0, 2, 4, 6, 8]]:
        s0 = eng.pcg_sum_stats()
        eng.sync()
        t0 = time.perf_counter()
        val = obj.cv_solve(float(w))
        dt = time.perf_counter() - t0
        s1 = eng.pcg_sum_stats()
        obj.clear_res()
        print(f"| {w:.3f} | {val:.5e} | {dt:.2f} | {s1['solves'] - s0['solves']} | {s1['iterations'] - s0['iterations']} | "
              f"{s1['host_waits'] - s0['host_waits']} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["10x4", "64x4", "64x16"])
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-spectrum", action="store_true")
    args = ap.parse_args()
    eng = get_engine()
    print(f"### one CG iteration, {args.iters} iterations per solve, median of {args.repeats} solves (min - max)\n")
    print("| D | d | elements | three-term us / iteration | M1 us | M2 us | M3 us | vector kernels + launch gaps us | "
          "combined-MPO baseline us / iteration | baseline / three-term |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for s in args.sizes:
        D, d = [int(v) for v in s.split("x")]
        r = probe_size(eng, D, d, args.iters, args.repeats)
        us = lambda t: f"{t * 1e6:.0f}"
        rest = r["per_sum"] - sum(r["applies"])
        print(f"| {D} | {d} | {r['n']} | {us(r['per_sum'])} ({us(r['spread_sum'][0])} - {us(r['spread_sum'][1])}) | "
              f"{us(r['applies'][0])} | {us(r['applies'][1])} | {us(r['applies'][2])} | {us(rest)} | "
              f"{us(r['per_base'])} ({us(r['spread_base'][0])} - {us(r['spread_base'][1])}) | "
              f"{r['per_base'] / r['per_sum']:.2f} |", flush=True)
        if r["iters"][0] != args.iters or r["iters"][1] != args.iters:
            print(f"(iterations run: {r['iters']}, status {r['status']})")
    if not args.no_spectrum:
        spectrum_times()


if __name__ == "__main__":
    main()
