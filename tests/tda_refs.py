"""NumPy restatement of the tangent-space (TDA) operator of include/mpsengine.h (mpse_tda_*), the reference of
tests/test_tda_gpu.py; tests/test_tda_refs_host.py holds it against dense matrices without a GPU.

  gauge       from a chain of site arrays: the right-canonical sites B of the normalised state, the left-canonical sites A
              of the left-to-right SVD sweep and the tangent factors U (None where a site has no tangent space)
  dense_p     the tangent-space basis as a dense matrix P (columns in the order of the vector x)
  dense_h     the MPO as a dense matrix
  recursion   y = P^H H P x in 4 (N - 1) environment updates and 3 N effective-Hamiltonian applications
  hdiag       diag(P^H H P), site by site
Sites are (Dl, d, Dr), MPO sites (wl, d_up, d_down, wr), environments (bra bond, w, ket bond); x is the concatenation
of X_i (n_i, Dr_i), row major, over the sites that have a U_i."""
import numpy as np

from contract_refs import ref_env, ref_heff          # (tests/contract_refs.py)


def gauge(sites, include_psi0=False):
    """(A, B, U) of the chain ``sites``.  Every bond must be full on both sides (Dr <= Dl d and Dl <= d Dr), so that no
    shape changes; the state is normalised on the way."""
    n = len(sites)
    B = [np.array(s) for s in sites]
    for j in range(n - 1, -1, -1):                     # right-canonical, QR from the right
        dl, d, dr = B[j].shape
        q, r = np.linalg.qr(B[j].reshape(dl, d * dr).conj().T)      # M^H = q r  ->  M = r^H q^H
        assert q.shape[1] == dl, "a bond is not full"
        B[j] = q.conj().T.reshape(dl, d, dr)
        if j:
            B[j - 1] = np.tensordot(B[j - 1], r.conj().T, axes=(2, 0))
    A, U = [], []
    c = B[0]
    for j in range(n):
        dl, d, dr = c.shape
        u, s, vt = np.linalg.svd(c.reshape(dl * d, dr), full_matrices=True)
        rank = len(s)
        assert rank == dr, "a bond is not full"
        if include_psi0 and j == n - 1:
            U.append(u.reshape(dl, d, -1))
        else:
            U.append(u[:, rank:].reshape(dl, d, -1) if rank < u.shape[1] else None)
        A.append(u[:, :rank].reshape(dl, d, rank))
        if j < n - 1:
            c = np.tensordot(s[:, None] * vt, B[j + 1], axes=(1, 0))
    return A, B, U


def xshapes(B, U):
    return [None if u is None else (u.shape[2], B[j].shape[2]) for j, u in enumerate(U)]


def xsize(B, U):
    return sum(s[0] * s[1] for s in xshapes(B, U) if s is not None)


def split_x(x, B, U):
    out, off = [], 0
    for s in xshapes(B, U):
        if s is None:
            out.append(None)
        else:
            out.append(x[off:off + s[0] * s[1]].reshape(s))
            off += s[0] * s[1]
    assert off == len(x)
    return out


def dense_p(A, B, U):
    """P (prod d, xsize): column (j, l, r) is A_0 .. A_{j-1} U_j[:, :, l] (x) e_r B_{j+1} .. B_{N-1}"""
    n = len(A)
    left = [np.ones((1, 1))]                           # (physical indices so far, bond)
    for j in range(n - 1):
        t = np.tensordot(left[-1], A[j], axes=(1, 0))
        left.append(t.reshape(-1, t.shape[-1]))
    right = [None] * (n + 1)
    right[n] = np.ones((1, 1))                         # (bond, physical indices behind)
    for j in range(n - 1, 0, -1):
        t = np.tensordot(B[j], right[j + 1], axes=(2, 0))
        right[j] = t.reshape(t.shape[0], -1)
    cols = []
    for j in range(n):
        if U[j] is None:
            continue
        t = np.tensordot(left[j], U[j], axes=(1, 0))                  # PL, d, n
        t = np.einsum("pdl,rq->pdqlr", t, right[j + 1])               # PL, d, PR, n, Dr
        cols.append(t.reshape(-1, U[j].shape[2] * B[j].shape[2]))
    return np.concatenate(cols, axis=1)


def dense_h(W):
    """the MPO as a matrix, rows the up legs (which meet the bra)"""
    t = np.ones((1, 1, 1))                             # up, down, bond
    for w in W:
        t = np.einsum("udb,bxyc->uxdyc", t, w)
        t = t.reshape(t.shape[0] * t.shape[1], t.shape[2] * t.shape[3], t.shape[4])
    return t[:, :, 0]


def const_envs(A, B, W):
    """L_0 .. L_N from the A, R_0 .. R_N from the B"""
    n = len(A)
    L = [np.ones((1, 1, 1))]
    for j in range(n):
        L.append(ref_env("L", L[-1], A[j], W[j]))
    R = [None] * (n + 1)
    R[n] = np.ones((1, 1, 1))
    for j in range(n - 1, -1, -1):
        R[j] = ref_env("R", R[j + 1], B[j], W[j])
    return L, R


def recursion(A, B, U, W, x, counts=None):
    """y = P^H H P x; counts (a dict) receives the number of environment updates and effective-Hamiltonian applications"""
    n = len(A)
    L, R = const_envs(A, B, W)
    X = split_x(np.asarray(x), B, U)
    T = [None if U[j] is None else np.tensordot(U[j], X[j], axes=(2, 0)) for j in range(n)]
    nenv = nheff = 0
    F = [None] * (n + 1)
    for j in range(n - 1):
        f = None
        if F[j] is not None:
            f = ref_env("L", F[j], B[j], W[j], bra=A[j])
            nenv += 1
        if T[j] is not None:
            g = ref_env("L", L[j], T[j], W[j], bra=A[j])
            nenv += 1
            f = g if f is None else f + g
        F[j + 1] = f
    G = [None] * (n + 1)
    for j in range(n - 1, 0, -1):
        f = None
        if G[j + 1] is not None:
            f = ref_env("R", G[j + 1], A[j], W[j], bra=B[j])
            nenv += 1
        if T[j] is not None:
            g = ref_env("R", R[j + 1], T[j], W[j], bra=B[j])
            nenv += 1
            f = g if f is None else f + g
        G[j] = f
    out = []
    for j in range(n):
        if U[j] is None:
            continue
        o = ref_heff(L[j], R[j + 1], [W[j]], T[j])
        nheff += 1
        if F[j] is not None:
            o = o + ref_heff(F[j], R[j + 1], [W[j]], B[j])
            nheff += 1
        if G[j + 1] is not None:
            o = o + ref_heff(L[j], G[j + 1], [W[j]], A[j])
            nheff += 1
        out.append(np.tensordot(U[j].conj(), o, axes=([0, 1], [0, 1])).ravel())
    if counts is not None:
        counts["env"], counts["heff"] = nenv, nheff
    return np.concatenate(out)


def hdiag(A, B, U, W):
    """diag(P^H H P): hdiag_j[l, r] = sum conj(U[a,g,l]) L[a,b,c] U[c,h,l] W[b,g,h,e] R[r,e,r]"""
    L, R = const_envs(A, B, W)
    out = []
    for j, u in enumerate(U):
        if u is None:
            continue
        rd = np.einsum("rer->re", R[j + 1])
        out.append(np.einsum("agl,abc,chl,bghe,re->lr", u.conj(), L[j], u, W[j], rd, optimize=True).ravel())
    return np.concatenate(out).real


def hnorm_bound(W):
    """prod |W_i|_F >= |H|_2: A, B and U are isometries, so it also bounds |P^H H P|_2"""
    return float(np.prod([np.linalg.norm(w.ravel()) for w in W]))


# the engine-level cases of tests/test_tda_gpu.py: state bonds, physical dims, MPO bonds, include_psi0
CASES = {
    "edge": ((1, 2, 4, 3, 1), (2, 3, 2, 3), (1, 3, 4, 2, 1), False),
    "two_sites": ((1, 2, 1), (2, 3), (1, 2, 1), False),
    "gap_site": ((1, 2, 4, 2, 1), (2, 2, 2, 2), (1, 2, 1, 2, 1), False),
    "bond17": ((1, 3, 9, 17, 9, 3, 1), (3, 3, 2, 3, 3, 3), (1, 5, 9, 8, 9, 5, 1), False),
    "edge_psi0": ((1, 2, 4, 3, 1), (2, 3, 2, 3), (1, 3, 4, 2, 1), True),
}
KINDS = {"real": (False, False), "cplx_state": (True, False), "cplx_both": (True, True)}


def problem(case, kind, seed=20240611):
    """(A, B, U, W) of a case in one of the three kinds, seeded through tests/chain_problems.py"""
    from chain_problems import _chain, _mpo          # (tests/chain_problems.py)
    bonds, ds, wb, psi0 = CASES[case]
    cs, cw = KINDS[kind]
    rng = np.random.default_rng(seed)
    sites = _chain(rng, bonds, ds, cs)
    W = _mpo(rng, wb, ds, cw)
    A, B, U = gauge(sites, include_psi0=psi0)
    return A, B, U, W
