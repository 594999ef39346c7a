#!/usr/bin/env python3
"""Prints one sha256 of the raw bytes of x plus (status, iters) per case of ``mpse_pcg``, ``mpse_pcg_sum`` and
``mpse_pcg_batch``, for a fixed list of seeded problems, on one GPU.

    python tools/pcg_bits.py [out.txt]

Two libraries of one ABI compute the same bits when their outputs are the same text: run it once per library
(RENO_MPSENGINE selects one) on the same machine and compare.  The order of every sum of a solve is fixed, so a line
depends on the inputs and the code alone.  The problems and the helpers are those of tests/test_pcg_gpu.py,
tests/test_pcg_sum_gpu.py and tests/test_pcg_batch_gpu.py."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import test_pcg_batch_gpu as TB
    import test_pcg_gpu as T
    import test_pcg_sum_gpu as TS
    from renormalizer_amd.engine import get_engine
    eng = get_engine()
    lines = []

    def emit(label, x, res):
        digest = hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
        lines.append(f"{label:52s} status {res.status} iters {res.iters:4d} {digest} {res.relres!r} {res.lvalue!r}")
        print(lines[-1], flush=True)

    # mpse_pcg: one and two layers, one- and two-site, real and complex, masked and not, with and without diag
    for dims, site in ((T.ONE_SMALL, "1site"), (T.TWO_SMALL, "2site")):
        for two in (False, True):
            for cplx in (False, True):
                for masked in (False, True):
                    p = T.Problem(eng, 11, dims, cplx, two, masked)
                    b, x0 = p.rhs(5)
                    for precond in (False, True):
                        res, dx, _, _ = p.solve(b, x0, 1e-8, precond)
                        emit(f"pcg {site} layers={1 + two} {'c128' if cplx else 'f64'} mask={int(masked)} "
                             f"diag={int(precond)}", dx.to_host(), res)
    # a right-hand side that vanishes under the mask
    p = T.Problem(eng, 41, T.ONE_SMALL, False, False, True)
    _, x0 = p.rhs(1)
    b = (T._rand(np.random.default_rng(2), p.shape, False) * ~p.mask).ravel()
    res, dx, _, _ = p.solve(b, x0, 1e-8)
    emit("pcg zero rhs", dx.to_host(), res)
    # max_iter = 1
    for two in (False, True):
        p = T.Problem(eng, 51, T.ONE_SMALL, False, two, False)
        b, _ = p.rhs(3)
        res, dx, _, _ = p.solve(b, np.zeros_like(b), 1e-10, precond=True, max_iter=1)
        emit(f"pcg max_iter=1 layers={1 + two}", dx.to_host(), res)
    # indefinite operators: at the first curvature, and after one iteration
    p = T.Problem(eng, 61, T.ONE_SMALL, False, False, False)
    lam, _ = p.k.spectrum()
    b, x0 = p.rhs(4)
    res, dx, _, _ = p.solve(b, x0, 1e-8, check=False, shift=-(lam[-1] + 1.0))
    emit("pcg indefinite at once", dx.to_host(), res)
    p = T.Problem(eng, 62, T.ONE_SMALL, False, False, False)
    lam, idx = p.lam_h, p.lam_idx
    b = (p.k.vector(idx[-1]) + 0.3 * p.k.vector(idx[0])).astype(np.float64)
    res, dx, _, _ = p.solve(b, np.zeros_like(b), 1e-12, check=False, shift=-0.5 * (lam[0] + lam[-1]))
    emit("pcg indefinite after one", dx.to_host(), res)

    # mpse_pcg_sum: three terms; one term of weight 1 (the plain solve on its result) and of weight 2
    for name, dims, cplx, masked, precond in TS.CASES[:4]:
        sp = TS.SumProblem(eng, 11, dims, cplx, masked)
        b, x0 = sp.p.rhs(5)
        res, dx, _, _ = sp.solve(b, x0, 1e-8, precond)
        emit(f"pcg_sum three terms {name}", dx.to_host(), res)
    for cplx in (False, True):
        p = T.Problem(eng, 31, (23, 11, 29), cplx, True, True)
        b, x0 = p.rhs(7)
        Dl, d, Dr = p.shape
        hop = p.hop
        term = eng.ft_term(hop.cmo[0], hop.cmo[0], TS.UP, TS.UP, 1, 1, (Dl, d, 1, Dr), hop.l, hop.r)
        for w in (1.0, 2.0):
            db, dx = eng.asdevice(b.reshape(Dl, d, 1, Dr)), eng.asdevice(x0.reshape(Dl, d, 1, Dr))
            dd = eng.asdevice((w * (p.diag() - p.shift) + p.shift).reshape(Dl, d, 1, Dr))
            res = eng.pcg_sum([term], [w], db, dx, diag=dd, mask=p.dmask, shift=p.shift, tol=1e-8)
            emit(f"pcg_sum one term weight {w:g} {'c128' if cplx else 'f64'}", dx.to_host(), res)

    # mpse_pcg_batch
    def batch(label, members, **kw):
        res, xs, st = TB.solve(eng, members, **kw)
        for i, (r, x) in enumerate(zip(res, xs)):
            emit(f"{label} member {i} sets={st['launch_sets']} single={st['single_members']}", x, r)

    dims, w = (5, 3, 7), 3
    limit = eng.pcg_batch_stats()["set_limit"]
    me = TB.Member(eng, 41, dims, w, True, True, domega=0.07)
    others = [TB.Member(eng, 300 + i, dims, w, True, True, domega=0.02 * i, shift=0.25 + 0.05 * i) for i in range(4)]
    batch("batch alone", [me])
    batch("batch five", others[:2] + [me] + others[2:])
    batch("batch limit+1", [others[i % 4] for i in range(limit)] + [me])
    dims, w = (17, 4, 33), 5
    healthy = TB.Member(eng, 61, dims, w, False, True, shift=200.0)
    zero_b = TB.Member(eng, 62, dims, w, False, True)
    zero_b.b = (T._rand(np.random.default_rng(1), dims, False) * (1 - zero_b.p.mask)).ravel()
    slow = TB.Member(eng, 63, dims, w, False, True, shift=1e-4)
    bad = TB.Member(eng, 64, dims, w, False, True)
    bad.diag = bad.diag.copy()
    bad.diag[bad.diag.size // 2] = -1.0
    batch("batch ends differently", [healthy, zero_b, slow, bad], tol=1e-5, max_iter=3)
    a = [TB.Member(eng, 70 + i, (5, 3, 7), 3, False, True, domega=0.1 * i) for i in range(2)]
    c = [TB.Member(eng, 80 + i, (17, 4, 33), 5, False, False, domega=0.1 * i) for i in range(2)]
    out = TB.Member(eng, 90, (5, TB.SM2_DMAX + 1, 4), 3, False, True)
    batch("batch mixed", [a[0], c[0], out, a[1], c[1]])

    text = "\n".join(lines) + "\n"
    print("sha256 of all lines:", hashlib.sha256(text.encode()).hexdigest())
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
