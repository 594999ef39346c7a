#!/usr/bin/env python3
"""Times SpectraZtCV.cv_solve for one frequency of the headline chain (25 molecules, N = 50 sites, d = 2 / 16) at
m_max = 32 and 64: per centre the time of the engine's conjugate gradients (mpse_pcg), its iterations, host waits and
the matvecs enqueued past the decision, and for every ``--every``-th centre the same system through a conjugate
gradients loop driven from the host (Hop, mpse_dotc, mpse_axpy, mpse_mul_real: two dots and a norm read back per
iteration) - the only baseline there is.  Prints a markdown table per m_max.  Not part of bench.py.

    python tools/cv_probe.py [--m-max 32 64] [--omega 0.0] [--eta 5e-3] [--sweeps 3] [--every 5]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity  # noqa: E402
from renormalizer_amd.cv import SpectraZtCV  # noqa: E402
from renormalizer_amd.engine import get_engine  # noqa: E402
from renormalizer_amd.mps.mps import Mps  # noqa: E402


def host_cg(eng, hop, b, x, diag, mask, shift, tol, max_iter):
    lib, ctx = eng.lib, eng.ctx
    inv = eng.asdevice(1.0 / diag.to_host())

    def amul(v):
        y = hop(v)
        eng._check(lib.mpse_mul_real(ctx, y.code, y.ptr, mask.ptr, y.size))
        eng._check(lib.mpse_axpy(ctx, y.code, y.ptr, v.ptr, y.size, shift, 0.0))
        return y

    def axpy(y, v, a):
        eng._check(lib.mpse_axpy(ctx, y.code, y.ptr, v.ptr, y.size, float(a), 0.0))

    def prec(r):
        z = r.copy()
        eng._check(lib.mpse_mul_real(ctx, z.code, z.ptr, inv.ptr, z.size))
        return z

    rd = lambda a, c: complex(a.vdot(c)).real
    b = b.copy()
    eng._check(lib.mpse_mul_real(ctx, b.code, b.ptr, mask.ptr, b.size))
    eng._check(lib.mpse_mul_real(ctx, x.code, x.ptr, mask.ptr, x.size))
    r = b.copy()
    axpy(r, amul(x), -1.0)
    z = prec(r)
    p = z.copy()
    rz, bb, k = rd(r, z), rd(b, b), 0
    while rd(r, r) > tol * tol * bb and k < max_iter:
        q = amul(p)
        alpha = rz / rd(p, q)
        axpy(x, p, alpha)
        axpy(r, q, -alpha)
        z = prec(r)
        rz_new = rd(r, z)
        axpy(z, p, rz_new / rz)
        p, rz, k = z, rz_new, k + 1
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m-max", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--omega", type=float, default=0.0)
    ap.add_argument("--eta", type=float, default=5e-3)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--nmol", type=int, default=25)
    args = ap.parse_args()
    eng = get_engine()
    ph = Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.274571056529368), 16)
    model = HolsteinModel([Mol(Quantity(0.0), [ph], 1.0)] * args.nmol, Quantity(3.0e-2), 3)
    h_mpo = Mpo(model)
    gs = Mps.ground_state(model, False)
    e0 = gs.expectation(h_mpo)
    b_mps = Mpo.onsite(model, r"a^\dagger", dipole=True).apply(gs.scale(-args.eta))
    procedure = ([0.4, 0.2] + [0] * 50)[:args.sweeps]
    for m_max in args.m_max:
        cv0 = Mps.random(model, b_mps.qntot, m_max, percent=1.0, rng=np.random.default_rng(11))
        obj = SpectraZtCV(model, "abs", m_max, args.eta, h_mpo=h_mpo, procedure_cv=procedure, b_mps=b_mps, e0=e0,
                          cv_mps=cv0)
        rows = []
        pcg = eng.pcg

        def timed(hop, b, x, diag=None, mask=None, shift=0.0, tol=1e-5, max_iter=0, check=True):
            host = None
            if len(rows) % args.every == 0:
                xh = x.copy()
                eng.sync()
                t0 = time.perf_counter()
                kh = host_cg(eng, hop, b, xh, diag, mask, shift, tol, 10 * x.size)
                eng.sync()
                host = (time.perf_counter() - t0, kh)
            s0 = eng.pcg_stats()
            eng.sync()
            t0 = time.perf_counter()
            res = pcg(hop, b, x, diag=diag, mask=mask, shift=shift, tol=tol, max_iter=max_iter, check=check)
            dt = time.perf_counter() - t0
            s1 = eng.pcg_stats()
            rows.append((x.shape, x.size, dt, res.iters, s1["host_waits"] - s0["host_waits"],
                         s1["matvecs"] - s0["matvecs"] - res.iters, res.status, host))
            return res

        eng.pcg = timed
        try:
            t0 = time.perf_counter()
            val = obj.cv_solve(args.omega)
            wall = time.perf_counter() - t0
        finally:
            eng.pcg = pcg
        t_solve = sum(r[2] for r in rows)
        t_base = sum(r[7][0] for r in rows if r[7])
        print(f"\n### m_max = {m_max}: omega = {args.omega}, eta = {args.eta}, {len(procedure)} sweeps, {len(rows)} centres, "
              f"spectral value {val:.6e}")
        print(f"cv_solve {wall:.2f} s wall, of which host-driven baseline solves {t_base:.2f} s and mpse_pcg {t_solve:.2f} s; "
              f"iterations {sum(r[3] for r in rows)}, host waits {sum(r[4] for r in rows)}, matvecs past the decision "
              f"{sum(r[5] for r in rows)}, not converged {sum(1 for r in rows if r[6] != 0)}\n")
        print("| centre | shape | elements | mpse_pcg ms | iterations | us / iteration | host waits | wasted matvecs | "
              "host-driven ms | host-driven iterations | ratio |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for i, (shape, n, dt, it, waits, wasted, st, host) in enumerate(rows):
            if host is None:
                continue
            print(f"| {i} | {'x'.join(map(str, shape))} | {n} | {dt * 1e3:.2f} | {it} | {dt * 1e6 / max(it, 1):.0f} | {waits} | "
                  f"{wasted} | {host[0] * 1e3:.2f} | {host[1]} | {host[0] / dt:.2f} |")


if __name__ == "__main__":
    main()
