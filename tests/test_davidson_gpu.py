"""The Davidson eigensolver of the engine (mpse_davidson, through lib.davidson) and the inputs it feeds on (_hdiag,
mpse_heff_apply2, mpse_env_update_multi, mpse_davidson_precond), each against a float64 reference computed on the
host: np.linalg.eigh of the dense operator for centres of up to ~2000 elements, and Kronecker sums
H = A x 1 x 1 + 1 x B x 1 + 1 x 1 x C with a known spectrum where a dense eigh is out of reach."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import mps_oracle as orc
from renormalizer_amd import engine as E
from renormalizer_amd.lib.davidson import MAX_BASIS, MAX_ROOTS, davidson, davidson_multi, default_max_space
from renormalizer_amd.mps.gs import _hdiag
from renormalizer_amd.mps.hop_expr import hop_expr

from kron_problems import _rand, kron_problem   # (tests/kron_problems.py)

pytestmark = pytest.mark.gpu

TOL = 1e-12                                  # eigh_iterative's algo = "davidson"
PRIMME_TOL = -1e-6                           # algo = "primme": |r| < 1e-6 alone


def primme_space(nroots):
    return max(15, 2 * nroots + 7)


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


# ----------------------------------------------------------------------------------------------- operators

def _herm_env(rng, D, w, cplx, ramp=1.0):
    """(D, w, D): every channel (x + x^H) / 2 of a random x; channel 0 carries a diagonal ramp so that the diagonal
    preconditioner has something to work with (a sum-of-products Hamiltonian has its on-site terms there)"""
    x = _rand(rng, (D, w, D), cplx) / np.sqrt(D)
    x = (x + x.transpose(2, 1, 0).conj()) / 2
    x[:, 0, :] += np.diag(ramp * np.arange(D) / D)
    return x


def _sym_site(rng, wl, d, wr):
    """real MPO site (wl, d, d, wr), symmetric in its physical legs, identity in channel (0, 0)"""
    w = rng.standard_normal((wl, d, d, wr)) / d
    w = (w + w.transpose(0, 2, 1, 3)) / 2
    w[0, :, :, 0] = np.eye(d)
    return w


def dense_problem(seed, shape, w, cplx):
    """Hermitian centre problem from random environments: shape (Dl, d, Dr) or (Dl, d0, d1, Dr), MPO bonds w =
    (wl, wr) or (wl, wm, wr).  Returns (l, r, cmo)."""
    rng = np.random.default_rng(seed)
    Dl, Dr = shape[0], shape[-1]
    l = _herm_env(rng, Dl, w[0], cplx)
    r = _herm_env(rng, Dr, w[-1], cplx)
    ds = shape[1:-1]
    cmo = [_sym_site(rng, w[i], ds[i], w[i + 1]) for i in range(len(ds))]
    return l, r, cmo


# ----------------------------------------------------------------------------------------------- engine calls

def _hop(eng, l, r, cmo, cshape, twolayer=False):
    return hop_expr(eng.asdevice(l), eng.asdevice(r), [eng.asdevice(w) for w in cmo], cshape, twolayer)


def _guesses(eng, rng, shape, k, cplx, mask=None):
    out = []
    for _ in range(k):
        g = _rand(rng, shape, cplx)
        if mask is not None:
            g = g * mask
        out.append(eng.asdevice(g))
    return out


def _warm(eng, rng, vecs, shape, cplx, noise=0.05, mask=None):
    """start vectors: exact eigenvectors (columns of vecs) plus random vectors of relative norm ``noise`` (masked
    like the iteration) - the rotated roots of the previous centre that a DMRG sweep hands to the solver.  Close
    starts keep the cycle counts of these tests well under max_cycle; random starts are exercised by
    test_davidson_guesses and test_davidson_bitwise_reproducible."""
    out = []
    for i in range(vecs.shape[1]):
        z = _rand(rng, shape, cplx)
        if mask is not None:
            z = z * mask
        g = vecs[:, i].reshape(shape) + noise * z / np.linalg.norm(z)
        out.append(eng.asdevice(g.astype(np.complex128 if cplx else np.float64)))
    return out


def _solve(eng, hop, hdiag, nroots, guesses, mask=None, tol=TOL, max_space=None, max_cycle=100):
    """lib.davidson on a hop_expr operator; returns (e array, X (n, k) host, ncycle)"""
    md = None if mask is None else eng.asdevice(mask.astype(np.float64))
    if nroots == 1 and len(guesses) == 1:
        e, x, ncyc = davidson(hop, guesses[0], hdiag, mask=md, tol=tol, max_cycle=max_cycle,
                              max_space=12 if max_space is None else max_space)
        e, xs = [e], [x]
    else:
        e, xs, ncyc = davidson_multi(hop, guesses, hdiag, nroots, mask=md, tol=tol, max_cycle=max_cycle,
                                     max_space=max_space)
    X = np.stack([x.to_host().ravel() for x in xs], axis=1)
    return np.asarray(e), X, ncyc


def _raw(eng, hop, hdiag, nroots, guesses, mask=None, tol=TOL, max_space=0, max_cycle=100, lindep=1e-14):
    """mpse_davidson itself: (status, last error, e, X (n, nroots), ncycle, nmatvec)"""
    cplx = hop.operator_is_complex or any(g.is_complex for g in guesses)
    dt = np.complex128 if cplx else np.float64
    n = int(np.prod(hop.cshape))
    stack = eng.asdevice(np.stack([g.to_host().ravel().astype(dt) for g in guesses]))
    md = None if mask is None else eng.asdevice(mask.astype(np.float64))
    out = eng.zeros((nroots, n), dt)
    e = (C.c_double * nroots)()
    ncyc, nmv = C.c_int(), C.c_int()
    st = eng.lib.mpse_davidson(eng.ctx, stack.code, C.byref(hop.heff), int(hop.twolayer), hdiag.ptr,
                               None if md is None else md.ptr, nroots, len(guesses), stack.ptr, tol, max_cycle,
                               max_space, lindep, 1e-4, e, out.ptr, C.byref(ncyc), C.byref(nmv))
    msg = eng.lib.mpse_last_error(eng.ctx)
    msg = msg.decode() if msg else ""
    return st, msg, np.array(list(e)), out.to_host().T, ncyc.value, nmv.value


# ----------------------------------------------------------------------------------------------- checks

def check_eigenpairs(apply, e, X, exact, tol, mask=None, gap_floor=1e-2, vtol=1e-10):
    """e / X (n, k) from the solver against the ``exact`` ascending eigenvalues of the same operator:
    - Ritz values are upper bounds of the exact eigenvalues of the same rank (interlacing);
    - eigenvalues agree to ~|r|^2 / gap where the gaps to the rest of the spectrum are >= gap_floor;
    - |H x - e x| recomputed here meets the solver's own criterion;
    - the vectors are orthonormal, and exactly zero outside the mask."""
    k = len(e)
    assert X.shape[1] == k
    scale = max(1.0, np.abs(exact[: k + 1]).max())
    assert np.all(e >= exact[:k] - 1e-12 * scale), (e, exact[:k])
    res_bound = -tol if tol < 0 else np.sqrt(tol)
    for i in range(k):
        x = X[:, i]
        r = apply(x) - e[i] * x
        if mask is not None:
            r = r * mask.ravel()
        rn = np.linalg.norm(r)
        assert rn < res_bound + 1e-13 * scale, (i, rn, res_bound)
        gap = min(abs(exact[j] - exact[i]) for j in range(len(exact)) if j != i and abs(exact[j] - exact[i]) > 1e-9)
        if gap >= gap_floor and not any(abs(exact[j] - exact[i]) <= 1e-9 for j in range(len(exact)) if j != i):
            assert abs(e[i] - exact[i]) <= max(1e-9 * scale, 4 * rn * rn / gap), (i, e[i], exact[i], rn, gap)
        else:
            assert abs(e[i] - exact[i]) <= max(1e-9 * scale, 4 * rn * rn / gap_floor) + 2 * rn, (i, e[i], exact[i])
    g = X.conj().T @ X
    assert np.abs(g - np.eye(k)).max() < vtol, np.abs(g - np.eye(k)).max()
    if mask is not None:
        assert np.all(X[~mask.ravel().astype(bool)] == 0)


def subspace_distance(X, Y):
    """|P_X - P_Y|_2 for orthonormal columns X (n, k), Y (n, k)"""
    qx, _ = np.linalg.qr(X)
    qy, _ = np.linalg.qr(Y)
    s = np.linalg.svd(qx.conj().T @ qy, compute_uv=False)
    return float(np.sqrt(max(0.0, 1.0 - s.min() ** 2)))


def outside_distance(X, Y):
    """largest component of the columns of X (orthonormal) outside span(Y)"""
    qy, _ = np.linalg.qr(Y)
    return float(np.linalg.norm(X - qy @ (qy.conj().T @ X), 2))


# =============================================================================================== the operators

def test_kron_construction_matches_hop_dense():
    """Host-side premise of the Kronecker tests: the environment / MPO form of Kron is the Kronecker sum, one and two
    sites, and its eigenvalues are the sums of the factor eigenvalues."""
    for dims, cplx in (((5, 3, 4), True), ((4, 3, 2, 5), False), ((3, 2, 3, 4), True)):
        k = kron_problem(1, dims, cplx)
        h = orc.hop_dense(k.l, k.r, k.cmo)
        x = _rand(np.random.default_rng(0), (k.n,), cplx)
        assert np.abs(h @ x - k.apply(x)).max() < 1e-12
        assert np.abs(np.diag(h).real - k.diag()).max() < 1e-12
        assert np.abs(h - h.conj().T).max() < 1e-12
        vals, idx = k.spectrum()
        assert np.abs(np.linalg.eigvalsh(h) - vals).max() < 1e-11
        v = k.vector(idx[3])
        assert np.abs(h @ v - vals[3] * v).max() < 1e-11


def _square_env(e1):
    """two-layer environment of the square of a one-layer operator: L2[a,b,c,d] = sum_x L1[x,b,a] L1[d,c,x], and
    the same for R (a one-layer environment maps its last bond index to its first; a two-layer one takes the centre
    in through its first bond index and hands it out through its last, layer 1 acting first)"""
    return np.einsum("xba,dcx->abcd", e1, e1)


def test_two_layer_oracle_is_the_square():
    """hop_apply2 / hop_dense2 (written from the two-layer contraction) against the square of the one-layer oracle
    on environments built by _square_env, one and two sites."""
    for shape, w, cplx in (((5, 3, 4), (3, 2), True), ((3, 2, 3, 4), (2, 3, 2), False)):
        l1, r1, cmo = dense_problem(7, shape, w, cplx)
        h1 = orc.hop_dense(l1, r1, cmo)
        h2 = orc.hop_dense2(_square_env(l1), _square_env(r1), cmo)
        assert np.abs(h2 - h1 @ h1).max() < 1e-12 * np.abs(h2).max()
        c = _rand(np.random.default_rng(1), shape, cplx)
        out = orc.hop_apply2(_square_env(l1), _square_env(r1), cmo, c)
        assert np.abs(out.ravel() - h2 @ c.ravel()).max() < 1e-12 * np.abs(out).max()


# =============================================================================================== Davidson: dense

DENSE = [((13, 5, 19), (3, 4)), ((7, 3, 4, 11), (3, 2, 4))]     # 1235 / 924 elements, Dl != Dr


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("case", range(len(DENSE)))
@pytest.mark.parametrize("nroots", [1, 3, 10])
def test_davidson_dense_vs_eigh(eng, nroots, case, cplx):
    shape, w = DENSE[case]
    l, r, cmo = dense_problem(50 + case, shape, w, cplx)
    h = orc.hop_dense(l, r, cmo)
    exact, vecs = np.linalg.eigh(h)
    hop = _hop(eng, l, r, cmo, shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(nroots)
    e, X, ncyc = _solve(eng, hop, hd, nroots, _warm(eng, rng, vecs[:, :nroots], shape, cplx))
    assert len(e) == nroots and 0 < ncyc < 100
    check_eigenpairs(lambda x: h @ x, e, X, exact, TOL)


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_dense_mask(eng, cplx):
    """A charge mask: the reference is the eigh of the allowed block; the vectors are exactly zero elsewhere."""
    shape, w = DENSE[0]
    l, r, cmo = dense_problem(21, shape, w, cplx)
    q = [np.arange(s) % 3 for s in shape]
    mask = (q[0][:, None, None] + q[1][None, :, None] + q[2][None, None, :]) % 3 == 1
    h = orc.hop_dense(l, r, cmo)
    m = mask.ravel()
    exact, vb = np.linalg.eigh(h[np.ix_(m, m)])
    vecs = np.zeros((h.shape[0], 4), dtype=vb.dtype)
    vecs[m] = vb[:, :4]
    hop = _hop(eng, l, r, cmo, shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(3)
    for nroots in (1, 4):
        e, X, _ = _solve(eng, hop, hd, nroots, _warm(eng, rng, vecs[:, :nroots], shape, cplx, mask=mask), mask=mask)
        check_eigenpairs(lambda x: h @ x, e, X, exact, TOL, mask=mask)


# =============================================================================================== Davidson: Kronecker

KRON_ONE = (23, 11, 29)                 # 7337 elements
KRON_TWO = (9, 5, 6, 13)                # 3510 elements


def _kron_run(eng, k, nroots, cplx, tol=TOL, max_space=None, seed=0, mask=None, noise=0.05, allowed=None):
    hop = _hop(eng, k.l, k.r, k.cmo, k.shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(seed)
    _, idx = k.spectrum(allowed)
    vecs = np.stack([k.vector(t) for t in idx[:nroots]], axis=1)
    gs = _warm(eng, rng, vecs, k.shape, cplx, noise, mask)
    return _solve(eng, hop, hd, nroots, gs, mask=mask, tol=tol, max_space=max_space)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("nroots", [1, 3, 9, 10, 16])
def test_davidson_kron_nroots_default_space(eng, nroots, cplx):
    """Every nroots with the default space 12 + 3 (nroots - 1); nroots >= 10 needs more than 48 basis vectors."""
    dims = KRON_ONE if nroots % 2 else KRON_TWO
    k = kron_problem(30 + nroots, dims, cplx)
    exact, _ = k.spectrum()
    e, X, ncyc = _kron_run(eng, k, nroots, cplx)
    assert len(e) == nroots and 0 < ncyc < 100
    check_eigenpairs(k.apply, e, X, exact, TOL)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("nroots", [14, 16])
def test_davidson_kron_primme_space(eng, nroots, cplx):
    """algo = "primme": residual-only test |r| < 1e-6 and the space max(15, 2 nroots + 7)."""
    k = kron_problem(50 + nroots, KRON_TWO, cplx)
    exact, _ = k.spectrum()
    e, X, ncyc = _kron_run(eng, k, nroots, cplx, tol=PRIMME_TOL, max_space=primme_space(nroots))
    assert len(e) == nroots and 0 < ncyc < 100
    check_eigenpairs(k.apply, e, X, exact, PRIMME_TOL)


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_kron_above_reduction_block_cap(eng, cplx):
    """Dl = Dr = 136, d = 17 (complex) / 29 (real): 314 432 / 536 384 elements, more than 256 reduction blocks of
    2048 doubles in the Gram / Ritz passes (the grid is capped and every block strides)."""
    k = kron_problem(60, (136, 17 if cplx else 29, 136), cplx)
    assert k.n * (2 if cplx else 1) > 256 * 256 * 8
    exact, _ = k.spectrum()
    e, X, ncyc = _kron_run(eng, k, 3, cplx)
    assert 0 < ncyc < 100
    check_eigenpairs(k.apply, e, X, exact, TOL)


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_kron_degenerate_clusters(eng, cplx):
    """B with a repeated lowest eigenvalue: exact pairs at ranks 0-1 and 2-3 (the pair shifted by the next level of
    C).  nroots = 1 and 3 cut through a pair, nroots = 4 covers both: compare spanned subspaces, not vectors."""
    k = kron_problem(70, KRON_ONE, cplx, degenerate=(1, 0))
    exact, idx = k.spectrum()
    assert abs(exact[1] - exact[0]) < 1e-12 and abs(exact[3] - exact[2]) < 1e-12
    assert exact[2] - exact[1] > 1e-2 and exact[4] - exact[3] > 1e-2
    V = np.stack([k.vector(t) for t in idx[:4]], axis=1)
    # distances ~ |r| / gap
    e, X, _ = _kron_run(eng, k, 4, cplx)
    check_eigenpairs(k.apply, e, X, exact, TOL)
    assert subspace_distance(X, V) < 1e-3
    assert subspace_distance(X[:, :2], V[:, :2]) < 1e-3
    e, X, _ = _kron_run(eng, k, 3, cplx, seed=1)
    check_eigenpairs(k.apply, e, X, exact, TOL)
    assert subspace_distance(X[:, :2], V[:, :2]) < 1e-3
    assert outside_distance(X, V) < 1e-3
    e1, X1, _ = _kron_run(eng, k, 1, cplx, seed=2)
    assert abs(e1[0] - exact[0]) < 1e-9
    assert outside_distance(X1, V[:, :2]) < 1e-3
    # a repeated lowest level of A instead: nroots = 2 covers the lowest pair
    k2 = kron_problem(71, KRON_ONE, cplx, degenerate=(0, 0))
    ex2, id2 = k2.spectrum()
    nclus = int(np.sum(np.abs(ex2 - ex2[0]) < 1e-12))
    assert nclus == 2
    e2, X2, _ = _kron_run(eng, k2, 2, cplx, seed=3)
    check_eigenpairs(k2.apply, e2, X2, ex2, TOL)
    V2 = np.stack([k2.vector(t) for t in id2[:2]], axis=1)
    assert subspace_distance(X2, V2) < 1e-3


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_kron_mask_charge_sector(eng, cplx):
    """Block-diagonal factors under a charge rule q_a + q_s + q_b == Q: the exact sector spectrum is the set of
    allowed sums."""
    dims = KRON_ONE
    charges = [np.arange(n) % 3 for n in dims]
    k = kron_problem(80, dims, cplx, charges=charges)
    Q = 2
    mask = ((charges[0][:, None, None] + charges[1][None, :, None] + charges[2][None, None, :]) == Q)
    # eigenvector j of a block-diagonal factor lives in one charge block: its charge is that of its support
    qev = [np.array([ch[np.abs(u[:, j]).argmax()] for j in range(u.shape[1])]) for u, ch in zip(k.u, charges)]
    allowed = lambda t: qev[0][t[0]] + qev[1][t[1]] + qev[2][t[2]] == Q
    exact, _ = k.spectrum(allowed)
    for nroots in (1, 5):
        e, X, _ = _kron_run(eng, k, nroots, cplx, mask=mask, seed=nroots, allowed=allowed)
        check_eigenpairs(k.apply, e, X, exact, TOL, mask=mask)
        assert np.abs(e - exact[:nroots]).max() < 1e-9 * max(1.0, abs(exact[nroots]))


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_restarts(eng, cplx):
    """A space of 4 with one root and 3 roots in a space of 8: the run restarts many times and still converges to
    the exact eigenpairs."""
    k = kron_problem(90, KRON_ONE, cplx)
    exact, _ = k.spectrum()
    e, X, ncyc = _kron_run(eng, k, 1, cplx, max_space=4, noise=0.2)
    assert ncyc > 4
    check_eigenpairs(k.apply, e, X, exact, TOL)
    e, X, ncyc = _kron_run(eng, k, 3, cplx, max_space=8, noise=0.2)
    assert ncyc > 3
    check_eigenpairs(k.apply, e, X, exact, TOL)
    assert np.abs(e - exact[:3]).max() < 1e-9


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_max_cycle_exit(eng, cplx):
    """max_cycle = 2: two cycles are reported, the vectors are normalised Ritz vectors, the values upper bounds."""
    k = kron_problem(100, KRON_ONE, cplx, eps=1.0)
    exact, idx = k.spectrum()
    vecs = np.stack([k.vector(t) for t in idx[:3]], axis=1)
    hop = _hop(eng, k.l, k.r, k.cmo, k.shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(1)
    for nroots in (1, 3):
        st, msg, e, X, ncyc, nmv = _raw(eng, hop, hd, nroots, _warm(eng, rng, vecs[:, :nroots], k.shape, cplx, 2.0),
                                        max_cycle=2)
        assert st == E.MPSE_OK, msg
        assert ncyc == 2 and nmv > 0
        assert np.all(e >= exact[:nroots] - 1e-12)
        assert np.abs(e - exact[:nroots]).max() > 1e-9                      # not converged yet
        assert np.abs(X.conj().T @ X - np.eye(nroots)).max() < 1e-10
        for i in range(nroots):                                              # Ritz values of the returned vectors
            assert abs(np.vdot(X[:, i], k.apply(X[:, i])).real - e[i]) < 1e-9 * max(1.0, abs(e[i]))


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_fewer_allowed_states_than_roots(eng, cplx):
    """A mask that allows 5 entries and nroots = 8: exactly the 5 eigenpairs of the allowed block come back (the
    engine reports NaN for the rest, the Python layer drops them), the rest of x_out is zero."""
    shape, w = DENSE[0]
    l, r, cmo = dense_problem(110, shape, w, cplx)
    mask = np.zeros(shape, dtype=bool)
    allowed = [(0, 0, 0), (3, 1, 7), (12, 4, 18), (6, 2, 2), (9, 0, 11)]
    for t in allowed:
        mask[t] = True
    h = orc.hop_dense(l, r, cmo)
    m = mask.ravel()
    hb = h[np.ix_(m, m)]
    exact, evec = np.linalg.eigh(hb)
    hop = _hop(eng, l, r, cmo, shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(5)
    gs = _guesses(eng, rng, shape, 8, cplx, mask)
    st, msg, e_raw, X_raw, _, _ = _raw(eng, hop, hd, 8, gs, mask=mask)
    assert st == E.MPSE_OK, msg
    assert np.all(np.isfinite(e_raw[:5])) and np.all(np.isnan(e_raw[5:]))
    assert np.all(X_raw[:, 5:] == 0)
    e, X, _ = _solve(eng, hop, hd, 8, gs, mask=mask)
    assert len(e) == 5 and X.shape[1] == 5
    assert np.abs(e - exact).max() < 1e-10 * max(1.0, np.abs(exact).max())
    assert np.all(X[~m] == 0)
    for i in range(5):
        assert abs(abs(np.vdot(evec[:, i], X[m, i])) - 1.0) < 1e-10


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_guesses(eng, cplx):
    """Duplicated and linearly dependent guesses are dropped and the run converges; a guess entirely outside the
    mask is refused with MPSE_ERR_ARG and a message (an ordinary status, not a device fault)."""
    k = kron_problem(120, KRON_ONE, cplx)
    exact, idx = k.spectrum()
    vecs = np.stack([k.vector(t) for t in idx[:3]], axis=1)
    hop = _hop(eng, k.l, k.r, k.cmo, k.shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(6)
    a, b, c = [g.to_host() for g in _warm(eng, rng, vecs, k.shape, cplx)]
    gs = [eng.asdevice(x) for x in (a, a, 2.0 * a, a - 0.5 * b, b, np.zeros(k.shape), c)]
    e, X, ncyc = _solve(eng, hop, hd, 3, gs)
    assert len(e) == 3 and ncyc < 100
    check_eigenpairs(k.apply, e, X, exact, TOL)
    mask = np.zeros(k.shape, dtype=bool)
    mask[: k.shape[0] // 2] = True
    outside = np.where(mask, 0, a)
    st, msg, _, _, _, _ = _raw(eng, hop, hd, 1, [eng.asdevice(outside)], mask=mask)
    assert st == E.MPSE_ERR_ARG and "guess" in msg
    # the context is usable afterwards
    e, X, _ = _solve(eng, hop, hd, 1, [eng.asdevice(a)])
    assert abs(e[0] - exact[0]) < 1e-9


@pytest.mark.parametrize("cplx", [False, True])
def test_davidson_bitwise_reproducible(eng, cplx):
    k = kron_problem(130, KRON_TWO, cplx)
    hop = _hop(eng, k.l, k.r, k.cmo, k.shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(7)
    gs = _guesses(eng, rng, k.shape, 4, cplx)
    a = _raw(eng, hop, hd, 4, gs)
    b = _raw(eng, hop, hd, 4, gs)
    assert a[0] == b[0] == E.MPSE_OK
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4:] == b[4:]


def _kron_two_layer(seed, dims, cplx):
    """(H - omega)^2 of a Kron operator as a two-layer problem: omega sits between two exact eigenvalues, nearer the
    lower one, above the ground state and where the four lowest levels of (H - omega)^2 are >= 2e-3 apart.  Returns
    (kron, l2, r2, omega, sorted exact squared spectrum)."""
    k = kron_problem(seed, dims, cplx)
    vals, _ = k.spectrum()
    for rank in range(2, 40):
        omega = vals[rank] + 0.3 * (vals[rank + 1] - vals[rank])
        sq = np.sort((vals - omega) ** 2)
        if np.diff(sq[:4]).min() >= 2e-3:
            break
    l1 = k.l.copy()
    l1[:, 0, :] -= omega * np.eye(dims[0])
    l2 = _square_env(l1)
    r2 = _square_env(k.r)
    return k, l2, r2, omega, sq


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("dims", [(5, 4, 6), (4, 3, 3, 5)])
def test_davidson_two_layer_known_spectrum(eng, dims, cplx):
    k, l2, r2, omega, sq = _kron_two_layer(140, dims, cplx)
    assert np.diff(sq[:4]).min() >= 1e-3
    hop = _hop(eng, l2, r2, k.cmo, k.shape, twolayer=True)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo, twolayer=True)

    def apply(x):
        y = k.apply(x) - omega * x
        return k.apply(y) - omega * y

    rng = np.random.default_rng(8)
    _, idx = k.spectrum()
    vals = k.spectrum()[0]
    order = np.argsort((vals - omega) ** 2, kind="stable")
    vecs = np.stack([k.vector(idx[j]) for j in order[:3]], axis=1)
    for nroots in (1, 3):
        # the squared spectrum is narrow at the bottom and wide on top: a space of 24 keeps the run within 100 cycles
        e, X, ncyc = _solve(eng, hop, hd, nroots, _warm(eng, rng, vecs[:, :nroots], k.shape, cplx), max_space=24)
        assert ncyc < 100
        check_eigenpairs(apply, e, X, sq, TOL, gap_floor=1e-3)


def test_davidson_nroots_bound(eng):
    """nroots > 16 and a space that does not fit are refused: MPSE_ERR_ARG from the engine, ValueError naming the
    limit from the Python layer (eigh_iterative included) - no device work is attempted."""
    import types
    from renormalizer_amd.mps import gs
    from renormalizer_amd.utils import OptimizeConfig
    k = kron_problem(150, KRON_TWO, False)
    hop = _hop(eng, k.l, k.r, k.cmo, k.shape)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo)
    rng = np.random.default_rng(9)
    gs17 = _guesses(eng, rng, k.shape, 17, False)
    st, msg, _, _, _, _ = _raw(eng, hop, hd, 17, gs17)
    assert st == E.MPSE_ERR_ARG and "16" in msg
    st, msg, _, _, _, _ = _raw(eng, hop, hd, 4, gs17[:4], max_space=MAX_BASIS - 4)
    assert st == E.MPSE_ERR_ARG and "max_space" in msg
    with pytest.raises(ValueError, match=str(MAX_ROOTS)):
        davidson_multi(hop, gs17, hd, 17)
    with pytest.raises(ValueError, match=str(MAX_BASIS)):
        davidson_multi(hop, gs17[:4], hd, 4, max_space=MAX_BASIS - 4)
    assert default_max_space(MAX_ROOTS) + MAX_ROOTS + 1 <= MAX_BASIS
    assert primme_space(MAX_ROOTS) + MAX_ROOTS + 1 <= MAX_BASIS
    mps = types.SimpleNamespace(optimize_config=OptimizeConfig())
    mps.optimize_config.nroots = 17
    mask = np.ones(k.shape, dtype=bool)
    with pytest.raises(ValueError, match="16"):
        gs.eigh_iterative(mps, mask, hop.l, hop.r, hop.cmo, gs17, False)


# =============================================================================================== solver inputs

HDIAG_CASES = [((13, 5, 19), (3, 4)), ((7, 3, 4, 11), (3, 2, 4)), ((17, 2, 9), (1, 5)), ((5, 6, 3, 21), (4, 1, 3))]


@pytest.mark.parametrize("twolayer", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("case", range(len(HDIAG_CASES)))
def test_hdiag_vs_dense_diagonal(eng, case, cplx, twolayer):
    shape, w = HDIAG_CASES[case]
    l, r, cmo = dense_problem(200 + case, shape, w, cplx)
    if twolayer:
        rng = np.random.default_rng(case)
        # independent random two-layer environments: the diagonal does not need them to be squares
        l = _rand(rng, (shape[0], w[0], w[0], shape[0]), cplx)
        r = _rand(rng, (shape[-1], w[-1], w[-1], shape[-1]), cplx)
        ref = np.diag(orc.hop_dense2(l, r, cmo)).real
    else:
        ref = np.diag(orc.hop_dense(l, r, cmo)).real
    hop = _hop(eng, l, r, cmo, shape, twolayer)
    hd = _hdiag(eng, hop.l, hop.r, hop.cmo, twolayer)
    assert hd.dtype == np.float64 and hd.shape == shape
    out = hd.to_host().ravel()
    assert np.abs(out - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("cplx", [False, True])
def test_hdiag_kron_closed_form(eng, cplx):
    """At 314k elements (no dense operator): diag(A) x 1 x 1 + 1 x diag(B) x 1 + 1 x 1 x diag(C)."""
    k = kron_problem(210, (136, 17, 136), cplx)
    hop = _hop(eng, k.l, k.r, k.cmo, k.shape)
    out = _hdiag(eng, hop.l, hop.r, hop.cmo).to_host().ravel()
    ref = k.diag()
    assert np.abs(out - ref).max() < 1e-12 * np.abs(ref).max()
    k2 = kron_problem(211, (40, 6, 7, 44), cplx)
    hop = _hop(eng, k2.l, k2.r, k2.cmo, k2.shape)
    out = _hdiag(eng, hop.l, hop.r, hop.cmo).to_host().ravel()
    assert np.abs(out - k2.diag()).max() < 1e-12 * np.abs(k2.diag()).max()


HOP2_CASES = [((13, 3, 19), (3, 4)), ((21, 4, 10), (5, 2)), ((7, 3, 2, 11), (2, 3, 4)), ((17, 2, 3, 9), (4, 2, 3))]


def _heff2(eng, l, r, cmo, c):
    hop = _hop(eng, l, r, cmo, c.shape, twolayer=True)
    return hop(eng.asdevice(c)).to_host(), hop


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("case", range(len(HOP2_CASES)))
def test_heff_apply2_vs_oracle(eng, case, cplx):
    """mpse_heff_apply2 on random (not squared) two-layer environments, Dl != Dr, bonds off multiples of 16,
    wl != wm != wr; and the batched-identity form of Hop.dense() (danc / danc1 = n)."""
    shape, w = HOP2_CASES[case]
    rng = np.random.default_rng(300 + case)
    l = _rand(rng, (shape[0], w[0], w[0], shape[0]), cplx)
    r = _rand(rng, (shape[-1], w[-1], w[-1], shape[-1]), cplx)
    cmo = [rng.standard_normal((w[i], d, d, w[i + 1])) for i, d in enumerate(shape[1:-1])]
    c = _rand(rng, shape, cplx)
    ref = orc.hop_apply2(l, r, cmo, c)
    out, hop = _heff2(eng, l, r, cmo, c)
    assert np.abs(out - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())
    # a real centre with a complex operator is refused by the engine; a complex one with a real operator works
    if not cplx:
        cc = _rand(rng, shape, True)
        out, _ = _heff2(eng, l, r, cmo, cc)
        ref = orc.hop_apply2(l, r, cmo, cc)
        assert np.abs(out - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())
    dense = hop.dense()
    ref = orc.hop_dense2(l, r, cmo)
    assert np.abs(dense - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


def _multi_ref(env, ket, bra_c, mos, dom):
    """n-layer environment update by einsum: layer 1 touches the bra, layer n the ket; a 4-leg ket traces its
    ancilla against the bra's"""
    n = len(mos)
    letters = "bcde"[:n]
    anc = ket.ndim == 4
    phys = "xyzuv"
    if dom == "L":
        spec = ["a" + letters + "w", "a" + phys[0] + ("s" if anc else "") + "p"]
        spec += [letters[i] + phys[i] + phys[i + 1] + "FGHI"[i] for i in range(n)]
        spec += ["w" + phys[n] + ("s" if anc else "") + "q"]
        out = "p" + "FGHI"[:n] + "q"
    else:
        spec = ["a" + letters + "w", "p" + phys[0] + ("s" if anc else "") + "a"]
        spec += ["FGHI"[i] + phys[i] + phys[i + 1] + letters[i] for i in range(n)]
        spec += ["q" + phys[n] + ("s" if anc else "") + "w"]
        out = "p" + "FGHI"[:n] + "q"
    return np.einsum(",".join(spec) + "->" + out, env, bra_c, *mos, ket, optimize=True)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("dom", ["L", "R"])
@pytest.mark.parametrize("nlayer", [1, 2, 3, 4])
def test_env_update_multi_vs_einsum(eng, nlayer, dom, cplx):
    """mpse_env_update_multi against einsum: 1-4 layers, a separate bra with other bonds, bra_conj 0 / 1, 4-leg
    (ancilla) kets."""
    rng = np.random.default_rng(400 + nlayer)
    d = 3
    ws = [2, 3, 1, 4, 2][: nlayer + 1]
    mos = [rng.standard_normal((ws[i], d, d, ws[i + 1])) for i in range(nlayer)]
    for anc, sep, bra_conj in itertools.product((False, True), (False, True), (0, 1)):
        if not sep and not bra_conj:
            continue                                           # bra == ket is always conjugated here
        Dl, Dr = 9, 13
        BDl, BDr = (7, 17) if sep else (Dl, Dr)
        ket = _rand(rng, (Dl, d, 2, Dr) if anc else (Dl, d, Dr), cplx)
        bra = _rand(rng, (BDl, d, 2, BDr) if anc else (BDl, d, BDr), cplx) if sep else ket
        wl = tuple(m.shape[0] for m in mos)
        wr = tuple(m.shape[3] for m in mos)
        if dom == "L":
            env = _rand(rng, (BDl,) + wl + (Dl,), cplx)
            oshape = (BDr,) + wr + (Dr,)
        else:
            env = _rand(rng, (BDr,) + wr + (Dr,), cplx)
            oshape = (BDl,) + wl + (Dl,)
        bra_c = bra.conj() if bra_conj else bra
        ref = _multi_ref(env, ket, bra_c, mos, dom)
        dt = np.complex128 if cplx else np.float64
        dims = E.mpse_dims()
        dims.Dl_ket, dims.Dr_ket, dims.Dl_bra, dims.Dr_bra = Dl, Dr, BDl, BDr
        dims.d0, dims.d1, dims.danc = d, 1, 2 if anc else 1
        K, Bd, Ev = eng.asdevice(ket, dt), eng.asdevice(bra, dt), eng.asdevice(env, dt)
        Ws = [eng.asdevice(m) for m in mos]
        out = eng.empty(oshape, dt)
        wla, wra = (C.c_int64 * nlayer)(*wl), (C.c_int64 * nlayer)(*wr)
        ptrs = (C.c_void_p * nlayer)(*[w.ptr for w in Ws])
        eng._check(eng.lib.mpse_env_update_multi(eng.ctx, out.code, E.DOMAIN_L if dom == "L" else E.DOMAIN_R,
                                                 C.byref(dims), nlayer, wla, wra, Ev.ptr, Ev.code, K.ptr,
                                                 Bd.ptr if sep else None, bra_conj, ptrs, Ws[0].code, out.ptr))
        res = out.to_host()
        assert np.abs(res - ref).max() < 1e-12 * max(1.0, np.abs(ref).max()), (anc, sep, bra_conj)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 1000, 70001, 1048576 + 777])
def test_davidson_precond(eng, n, cplx):
    """out = r / (hdiag - e + shift), zero where the mask is 0; lengths off multiples of 256, and beyond the
    4096-block grid of the element-wise kernels."""
    rng = np.random.default_rng(n)
    r = _rand(rng, (n,), cplx)
    hd = rng.uniform(-3.0, 3.0, n)
    e, shift = 0.37, 1e-4
    mask = (rng.random(n) < 0.6).astype(np.float64)
    dt = np.complex128 if cplx else np.float64
    R, H, M = eng.asdevice(r), eng.asdevice(hd), eng.asdevice(mask)
    ref = r / (hd - e + shift)
    for m in (None, M):
        out = eng.empty((n,), dt)
        eng._check(eng.lib.mpse_davidson_precond(eng.ctx, out.code, out.ptr, R.ptr, H.ptr,
                                                 None if m is None else m.ptr, n, e, shift))
        res = out.to_host()
        want = ref if m is None else np.where(mask == 0, 0, ref)
        assert np.all(np.abs(res - want) <= 1e-15 * np.abs(want))
        if m is not None:
            assert np.all(res[mask == 0] == 0)
