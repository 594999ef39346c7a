#!/usr/bin/env python3
"""Prints one sha256 of the raw result bytes plus the Krylov dimension per case of ``mpse_expm_lanczos`` and
``mpse_expm_lanczos_batch``, for a fixed list of seeded problems, on one GPU.

    python tools/lanczos_bits.py [out.txt]

Two libraries of one ABI compute the same bits when their outputs are the same text: run it once per library
(RENO_MPSENGINE selects one) on the same machine and compare.  The order of every sum of a solve is fixed, so a line
depends on the inputs and the code alone.  The problems and the helpers are those of tests/test_lanczos_gpu.py: single
solves, real and complex, at n = 360 and n = 2040; a centre with a structural mask; the fused 0-site matvec with its
tile-masked parts; large one-site matvecs whose result may come in two parts; a breakdown; need_host at a later check;
the 64-vector limit; out == C; the batched cases of the tests."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import test_lanczos_gpu as T
    from renormalizer_amd.engine import get_engine
    from renormalizer_amd.mps.hop_expr import centre_tile_mask
    eng = get_engine()
    lines = []

    def emit(label, out, nv, extra=""):
        lines.append(f"{label:46s} nvec {nv:3d} {hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()} {extra}")
        print(lines[-1], flush=True)

    def single(label, k, hop, c, dt, rtol, atol=0.0, alias=False):
        dev = eng.asdevice(c)
        st, out, nv, d = T._solve(eng, hop, dev, dt, rtol, atol, out=dev if alias else None)
        assert st == 0, (label, st)
        emit(label, out, nv, " ".join(f"{a}={b}" for a, b in sorted(d.items()) if a.startswith("update_")))

    # single solves at the two sizes, real (imaginary time) and complex (real time), and out == C
    for dims, name in ((T.ASYNC_DIMS, "n360"), (T.LONG_DIMS, "n2040")):
        for cplx in (True, False):
            k = T.kron_problem(300, dims, cplx)
            c = T._rand(np.random.default_rng(1), (k.n,), cplx)
            width = sum(float(e.max() - e.min()) for e in k.ev)
            for tag, tau in (("short", 3.0 / width), ("long", 30.0 / width)):
                dt = -1j * tau if cplx else -tau
                single(f"single {name} {'c128' if cplx else 'f64'} {tag}", k, T._hop(k), c, dt, 1e-10, 1e-12)
            single(f"single {name} {'c128' if cplx else 'f64'} out==C", k, T._hop(k), c, dt, 1e-10, 1e-12, alias=True)
    # the 64-vector limit (hand-over to the synchronous solve), also with out == C
    k = T.kron_problem(300, T.LONG_DIMS, True)
    c = T._rand(np.random.default_rng(1), (k.n,), True)
    for alias in (False, True):
        single(f"vector limit alias={int(alias)}", k, T._hop(k), c, -1j * T.LONG_TAU, *T.LONG_TOL, alias=alias)
    # structural mask of the centre
    Dl, d, Dr = 32, 4, 64
    chl, chs, chr_ = np.arange(Dl) // 16, np.arange(d), np.arange(Dr) // 32
    k = T.kron_problem(130, (Dl, d, Dr), True, charges=[chl, chs, chr_])
    allowed = ((chl[:, None, None] + chs[None, :, None] + chr_[None, None, :]) == 1).reshape(Dl, d * Dr)
    hop = T._hop(k)
    hop.cmask = centre_tile_mask(eng, (chl[:, None] + chs[None, :]).reshape(-1, 1), chr_[:, None], np.array([1]), k.shape)
    c = (T._rand(np.random.default_rng(15), (Dl, d * Dr), True) * allowed).reshape(k.shape)
    for dt in (-0.3j, 0.2 - 0.1j):
        single(f"centre mask dt={dt}", k, hop, c, dt, 1e-10)
    # the matvec paths of the tests: a general solve and a breakdown (three exact eigenvectors) on each
    for name, dims, cplx, _ in T.MATVECS:
        k = T.kron_problem(60, dims, cplx)
        hop = T._hop(k)
        rng = np.random.default_rng(9)
        cb, lam, coef, U = T._eig_start(k, 3, rng, cplx)
        al, be = T._lanczos(k.apply, cb, 10)
        tau = 0.7 / T._gersh(al, be)
        single(f"matvec {name} breakdown", k, hop, cb.reshape(k.shape), -1j * tau if cplx else tau, 1e-14)
        g = T._rand(rng, k.shape, cplx)
        width = sum(float(e.max() - e.min()) for e in k.ev)
        single(f"matvec {name} general", k, hop, g, (-3j if cplx else -3.0) / width, 1e-10)
    # need_host at a later check, also with out == C
    k, c, dt = T._later_host_problem()
    for alias in (False, True):
        single(f"need_host later alias={int(alias)}", k, T._hop(k), c, dt, 1e-10, alias=alias)

    def batch(label, ks, cs, dt, rtol, atol, before=None):
        hops = [T._hop(k) for k in ks]
        for alias in (False, True):
            if before:
                before()
            devs = [eng.asdevice(c) for c in cs]
            st, outs, nvs, _, (nb, ns) = T._batch(eng, hops, devs, dt, rtol, atol, outs=devs if alias else None)
            assert st == 0, (label, st)
            for i, (o, nv) in enumerate(zip(outs, nvs)):
                emit(f"{label} alias={int(alias)} member {i}", o, nv, f"batched={nb} single={ns}")

    # the members of test_batched_members_across_bands
    k0 = T.kron_problem(80, T.ASYNC_DIMS, True)
    rng = np.random.default_rng(8)
    g = T._rand(rng, (k0.n,), True)
    al, be = T._lanczos(k0.apply, g, 30)
    g0 = T._gersh(al, be)
    tau = 0.35 / g0
    ks, cs = [], []
    for target in (0.0, 2.8, 11.3, 90.5, 362.0, 600.0):
        ks.append(T.kron_problem(80, T.ASYNC_DIMS, True, shift=0.0 if target == 0.0 else target / tau - g0))
        cs.append(T._rand(rng, (k0.n,), True))
    kb = T.kron_problem(81, T.ASYNC_DIMS, True)
    for kk in (2, 5, 8):
        ks.append(kb)
        cs.append(T._eig_start(kb, kk, rng, True)[0])
    batch("batch bands", ks, cs, -1j * tau, 1e-10, 0.0)
    # the members of test_batch_grows_and_member_leaves_at_limit, after a short solve of the class (capacity 16)
    base = [0.71, 0.43, 0.59, 0.37]
    k3 = T.kron_problem(300, T.LONG_DIMS, True)
    rng = np.random.default_rng(12)
    ks = [T.kron_problem(300, T.LONG_DIMS, True, shift=7.0, spacing=[0.12 * s for s in base]),
          T.kron_problem(300, T.LONG_DIMS, True, shift=3.0, spacing=[0.4 * s for s in base]), k3]
    cs = [T._rand(rng, (k3.n,), True), T._rand(rng, (k3.n,), True), T._rand(np.random.default_rng(1), (k3.n,), True)]
    cshort = T._eig_start(k3, 3, rng, True)[0]
    hop3 = T._hop(k3)

    def short_solve():
        st, _, nv, _ = T._solve(eng, hop3, eng.asdevice(cshort), -1j * T.LONG_TAU, 1e-14)
        assert st == 0 and nv <= 8, (st, nv)

    batch("batch grows", ks, cs, -1j * T.LONG_TAU, *T.LONG_TOL, before=short_solve)
    text = "\n".join(lines) + "\n"
    print("sha256 of all lines:", hashlib.sha256(text.encode()).hexdigest())
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
