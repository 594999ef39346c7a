"""The preconditioned conjugate gradients of the engine (mpse_pcg, through Engine.pcg) on centre problems whose solution
is known exactly: Kronecker sums H = A x 1 x 1 + 1 x B x 1 + 1 x 1 x R (tests/kron_problems.py), solved as H + s (one
layer) and as (H - omega)^2 + eta^2 (two stacked layers).  The exact x* = A^-1 b follows from the factor eigenvectors.

Every bound is derived, none is taken from what the solver gives:
  * returned |r| / |b| <= tol: the stopping rule itself;
  * |b - A x| recomputed outside the solver <= 2 tol |b|: the recurrence residual drifts from the true one by rounding,
    O(eps kappa) |b|, far below tol for the kappa used here; the factor 2 leaves room for it;
  * |x - x*| = |A^-1 r| <= |r| / lam_min and |b| <= lam_max |x*| give |x - x*| <= kappa tol |x*|, kappa = lam_max /
    lam_min of the shifted operator in the (masked) space, known exactly from the factor eigenvalues;
  * lvalue against Re(x^H A x) - 2 Re(b^H x) from the returned x: 1e-12 (|x^H A x| + |b^H x|), float64 sums of O(1e5) terms."""
import ctypes as C

import numpy as np
import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.mps.hop_expr import hop_expr

from kron_problems import Kron, _factor, _rand, kron_problem   # (tests/kron_problems.py)

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def k_wait(eng):
    """iterations between two host reads of the control block: the engine's own constant (mpse_pcg_stats entry 9)"""
    k = eng.pcg_stats()["wait_interval"]
    assert k >= 1
    return k


def _hop(eng, l, r, cmo, cshape, twolayer=False):
    return hop_expr(eng.asdevice(l), eng.asdevice(r), [eng.asdevice(w) for w in cmo], cshape, twolayer)


def _square_env(e1):
    """two-layer environment of the square of a one-layer operator (layer 1 acts first): L2[a,b,c,d] = sum_x L1[x,b,a]
    L1[d,c,x]"""
    return np.einsum("xba,dcx->abcd", e1, e1)


def _charges(dims):
    return [np.arange(n) % 3 for n in dims]


def _charge_mask(charges, Q):
    tot = 0
    for i, ch in enumerate(charges):
        shp = [1] * len(charges)
        shp[i] = len(ch)
        tot = tot + ch.reshape(shp)
    return tot == Q


class Problem:
    """A x = b with A = f(H) + shift on a Kron centre: one layer f(H) = H, two layers f(H) = (H - omega)^2.  Holds the
    device operator, the exact eigenvalues of A in the masked space and the exact solve."""

    def __init__(self, eng, seed, dims, cplx, twolayer, masked, shift=None, eta=0.5, width=5.0):
        charges = _charges(dims) if masked else None
        # level spacings that keep the spectrum of H about `width` wide whatever the factor sizes (kappa stays small)
        spacing = [width / (len(dims) * n) * (1.0 + 0.07 * i) for i, n in enumerate(dims)] + [0.0]
        k = kron_problem(seed, dims, cplx, charges=charges, spacing=spacing)
        self._setup(eng, k, cplx, twolayer, charges, shift, eta)

    @classmethod
    def from_kron(cls, eng, k, cplx, twolayer=False, charges=None, shift=None, eta=0.5):
        """the same problem around a ready Kron centre (``charges``: per factor, the factors must conserve them)"""
        p = cls.__new__(cls)
        p._setup(eng, k, cplx, twolayer, charges, shift, eta)
        return p

    def _setup(self, eng, k, cplx, twolayer, charges, shift, eta):
        self.eng, self.cplx, self.twolayer, self.k = eng, cplx, twolayer, k
        masked = charges is not None
        dims = k.shape
        self.shape, self.n = k.shape, k.n
        self.mask = None
        allowed = None
        if masked:
            Q = 2
            self.mask = _charge_mask(charges, Q)
            # eigenvector j of a block-diagonal factor lives in one charge block: its charge is that of its support
            qev = [np.array([ch[np.abs(u[:, j]).argmax()] for j in range(u.shape[1])]) for u, ch in zip(k.u, charges)]
            allowed = lambda t: sum(q[i] for q, i in zip(qev, t)) == Q
        lam, self.lam_idx = k.spectrum(allowed)
        self.lam_h = lam
        if twolayer:
            self.omega = 0.5 * (lam[0] + lam[-1]) + 0.01
            self.shift = eta * eta if shift is None else shift
            l1 = k.l.copy()
            l1[:, 0, :] -= self.omega * np.eye(dims[0])
            self.hop = _hop(eng, _square_env(l1), _square_env(k.r), k.cmo, k.shape, twolayer=True)
            self.lam_a = (lam - self.omega) ** 2 + self.shift
        else:
            self.omega = 0.0
            self.shift = 1.0 - lam[0] if shift is None else shift        # lowest eigenvalue of A: 1
            self.hop = _hop(eng, k.l, k.r, k.cmo, k.shape)
            self.lam_a = lam + self.shift
        self.kappa = self.lam_a.max() / self.lam_a.min()
        self.dtype = np.complex128 if cplx else np.float64
        self.dmask = None if self.mask is None else eng.asdevice(self.mask.astype(np.float64))

    def f_of_h(self, x):
        k = self.k
        if self.twolayer:
            y = k.apply(x) - self.omega * x
            return k.apply(y) - self.omega * y
        return k.apply(x)

    def apply(self, x):
        """A x on the host (x flat, inside the masked space)"""
        y = self.f_of_h(x)
        if self.mask is not None:
            y = y * self.mask.ravel()
        return y + self.shift * x

    def diag(self):
        """diagonal of A (float64, > 0 on the masked space when A is positive definite)"""
        k = self.k
        if not self.twolayer:
            return k.diag() + self.shift
        # diag((H - omega)^2)_i = sum_j |(H - omega)_ij|^2; for a Kronecker sum: (sum_f d_f - omega)^2 + sum_f offdiag_f
        d = k.diag() - self.omega
        off = 0
        for i, m in enumerate(k.f):
            o = (np.abs(m) ** 2).sum(axis=1) - np.abs(np.diag(m)) ** 2
            shp = [1] * len(k.shape)
            shp[i] = k.shape[i]
            off = off + o.reshape(shp)
        return d ** 2 + off.ravel() + self.shift

    def exact(self, b):
        """A^-1 b for a b inside the masked space (the factors conserve the charges, so A does)"""
        k = self.k
        y = k._each_factor(np.asarray(b, dtype=complex).reshape(k.shape), [u.conj().T for u in k.u])
        tot = sum(np.meshgrid(*k.ev, indexing="ij"))
        a = (tot - self.omega) ** 2 + self.shift if self.twolayer else tot + self.shift
        x = k._each_factor(y / a, k.u).ravel()
        return x if self.cplx else x.real

    def rhs(self, seed):
        rng = np.random.default_rng(seed)
        b = _rand(rng, self.shape, self.cplx)
        x0 = _rand(rng, self.shape, self.cplx)
        if self.mask is not None:
            b, x0 = b * self.mask, x0 * self.mask
        return b.astype(self.dtype).ravel(), x0.astype(self.dtype).ravel()

    def solve(self, b, x0, tol, precond=False, max_iter=0, check=True, shift=None):
        eng = self.eng
        db, dx = eng.asdevice(b.reshape(self.shape)), eng.asdevice(x0.reshape(self.shape))
        dd = eng.asdevice(self.diag().reshape(self.shape)) if precond else None
        s0 = eng.pcg_stats()
        res = eng.pcg(self.hop, db, dx, diag=dd, mask=self.dmask, shift=self.shift if shift is None else shift,
                      tol=tol, max_iter=max_iter, check=check)
        s1 = eng.pcg_stats()
        return res, dx, db, {key: s1[key] - s0[key] for key in s1}

    def device_residual(self, dx, db):
        """|b - A x| with Hop, mpse_mul_real and mpse_axpy, outside the solver"""
        eng = self.eng
        y = self.hop(dx)
        if self.dmask is not None:
            eng._check(eng.lib.mpse_mul_real(eng.ctx, y.code, y.ptr, self.dmask.ptr, y.size))
        eng._check(eng.lib.mpse_axpy(eng.ctx, y.code, y.ptr, dx.ptr, y.size, self.shift, 0.0))
        r = db.copy()
        eng._check(eng.lib.mpse_axpy(eng.ctx, r.code, r.ptr, y.ptr, r.size, -1.0, 0.0))
        return r.norm()


def host_driven_cg(p, b, x0, tol, precond, max_iter):
    """The same iteration driven from the host through the existing entry points (Hop, mpse_dotc, mpse_axpy,
    mpse_mul_real): two dots and a norm read back per iteration.  Returns (x host, iterations)."""
    eng = p.eng
    lib, ctx = eng.lib, eng.ctx

    def amul(v):
        y = p.hop(v)
        if p.dmask is not None:
            eng._check(lib.mpse_mul_real(ctx, y.code, y.ptr, p.dmask.ptr, y.size))
        eng._check(lib.mpse_axpy(ctx, y.code, y.ptr, v.ptr, y.size, p.shift, 0.0))
        return y

    def axpy(y, x, a):
        eng._check(lib.mpse_axpy(ctx, y.code, y.ptr, x.ptr, y.size, float(a), 0.0))

    def rdot(a, c):
        return complex(a.vdot(c)).real

    inv = eng.asdevice((1.0 / p.diag()).reshape(p.shape)) if precond else None

    def prec(r):
        z = r.copy()
        if inv is not None:
            eng._check(lib.mpse_mul_real(ctx, z.code, z.ptr, inv.ptr, z.size))
        return z

    db, x = eng.asdevice(b.reshape(p.shape)), eng.asdevice(x0.reshape(p.shape))
    r = db.copy()
    axpy(r, amul(x), -1.0)
    z = prec(r)
    pv = z.copy()
    rz, bb = rdot(r, z), rdot(db, db)
    k = 0
    while rdot(r, r) > tol * tol * bb and k < max_iter:
        q = amul(pv)
        alpha = rz / rdot(pv, q)
        axpy(x, pv, alpha)
        axpy(r, q, -alpha)
        z = prec(r)
        rz_new = rdot(r, z)
        axpy(z, pv, rz_new / rz)       # z + beta p
        pv, rz = z, rz_new
        k += 1
    return x.to_host().ravel(), k


# centre sizes on both sides of the one-launch small-centre matvec (32768 elements, one layer, one site) and one of
# more than 2^16 elements
ONE_SMALL, ONE_MID, ONE_BIG = (23, 11, 29), (48, 16, 48), (64, 17, 64)      # 7337, 36864, 69632 elements
TWO_SMALL, TWO_MID = (9, 5, 6, 13), (24, 8, 8, 24)                          # 3510, 36864 elements

CASES = [
    # (name, dims, complex environments, two layers, mask, preconditioner)
    ("one_small_f64", ONE_SMALL, False, False, False, False),
    ("one_small_c128_mask_pre", ONE_SMALL, True, False, True, True),
    ("one_mid_f64_mask", ONE_MID, False, False, True, False),
    ("one_mid_c128_pre", ONE_MID, True, False, False, True),
    ("one_big_f64_pre", ONE_BIG, False, False, False, True),
    ("two_site_f64_mask_pre", TWO_SMALL, False, False, True, True),
    ("two_site_c128", TWO_SMALL, True, False, False, False),
    ("two_site_mid_f64", TWO_MID, False, False, False, True),
    ("layer2_one_small_f64_mask_pre", ONE_SMALL, False, True, True, True),
    ("layer2_one_small_c128", ONE_SMALL, True, True, False, False),
    ("layer2_one_mid_f64_pre", ONE_MID, False, True, False, True),
    ("layer2_one_big_c128_mask_pre", ONE_BIG, True, True, True, True),
    ("layer2_two_site_f64_pre", TWO_SMALL, False, True, False, True),
    ("layer2_two_site_c128_mask", TWO_SMALL, True, True, True, False),
]


@pytest.mark.parametrize("tol", [1e-5, 1e-10])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pcg_exact_solution(eng, case, tol):
    name, dims, cplx, twolayer, masked, precond = case
    p = Problem(eng, 11, dims, cplx, twolayer, masked)
    assert p.lam_a.min() > 0
    b, x0 = p.rhs(5)
    xs = p.exact(b)
    res, dx, db, st = p.solve(b, x0, tol, precond)
    x = dx.to_host().ravel()
    nb = np.linalg.norm(b)
    true_res = p.device_residual(dx, db)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    ax = p.apply(x)
    xax, bx = np.vdot(x, ax).real, np.vdot(b, x).real
    direct = xax - 2 * bx
    print(f"{name} tol={tol:g}: n={p.n} kappa={p.kappa:.3g} iters={res.iters} relres={res.relres:.3e} "
          f"true={true_res / nb:.3e} err={err:.3e} (bound {p.kappa * tol:.3e}) lvalue dev={abs(res.lvalue - direct):.3e} "
          f"(bound {1e-12 * (abs(xax) + abs(bx)):.3e}) waits={st['host_waits']} matvecs={st['matvecs']}")
    assert res.status == 0
    assert res.relres <= tol
    assert true_res <= 2 * tol * nb
    assert err <= p.kappa * tol
    assert abs(res.lvalue - direct) <= 1e-12 * (abs(xax) + abs(bx))
    if masked:
        assert np.all(x[~p.mask.ravel()] == 0)
    assert st["solves"] == 1 and st["iterations"] == res.iters and st["end_tol"] == 1
    assert st["twolayer"] == int(twolayer) and st["masked"] == int(masked)
    assert 0 <= st["matvecs"] - st["iterations"] <= k_wait(eng) - 1


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_pcg_few_distinct_eigenvalues(eng, cplx, masked):
    """Exact-arithmetic property of the recurrence: with m distinct eigenvalues (here m = 6: {0, 1, 2} + {0} + {0, 10},
    shifted by 1) and no preconditioner, conjugate gradients end within m iterations; m + 2 allows for rounding."""
    dims = (12, 5, 14)
    rng = np.random.default_rng(3)
    charges = _charges(dims) if masked else [None] * 3
    levels = [np.repeat([0.0, 1.0, 2.0], 4), np.zeros(5), np.repeat([0.0, 10.0], 7)]
    if masked:
        # every level of a factor occurs in every charge block, so the masked space still holds all six sums
        levels = [np.array([0.0, 1.0, 2.0])[np.arange(12) // 3 % 3], np.zeros(5), np.array([0.0, 10.0])[np.arange(14) // 3 % 2]]
    fs = [_factor(rng, levels[i], cplx and i != 1, 0.3, charges[i]) for i in range(3)]
    p = Problem.from_kron(eng, Kron(fs, cplx), cplx, charges=charges if masked else None, shift=1.0)
    b, x0 = p.rhs(9)
    xs = p.exact(b)
    # the eigenvalues of A in the (masked) space the iteration runs in: 1, 2, 3, 11, 12, 13
    distinct = np.unique(np.round(p.lam_a, 9))
    assert len(distinct) == 6 and abs(p.kappa - 13.0) < 1e-9
    res, dx, _, _ = p.solve(b, x0, 1e-10)
    print(f"six eigenvalues, cplx={cplx} masked={masked}: iters={res.iters} relres={res.relres:.3e}")
    assert res.status == 0 and res.iters <= 6 + 2
    assert np.linalg.norm(dx.to_host().ravel() - xs) <= p.kappa * 1e-10 * np.linalg.norm(xs)


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[8], CASES[13]], ids=lambda c: c[0])
def test_pcg_decision_on_device(eng, case):
    """x is final at the deciding iteration: a second solve limited to the reported number of iterations (which the
    host stops enqueuing at) gives the same x bit for bit, and no more than K - 1 matvecs were enqueued past the decision."""
    name, dims, cplx, twolayer, masked, precond = case
    p = Problem(eng, 21, dims, cplx, twolayer, masked)
    b, x0 = p.rhs(6)
    res, dx, _, st = p.solve(b, x0, 1e-8, precond)
    assert res.status == 0 and res.iters > 0
    assert st["matvecs"] - st["iterations"] <= k_wait(eng) - 1
    res2, dx2, _, st2 = p.solve(b, x0, 1e-8, precond, max_iter=res.iters)
    assert res2.status == 0 and res2.iters == res.iters
    assert st2["matvecs"] == res.iters
    assert np.array_equal(dx.to_host(), dx2.to_host())
    assert res2.relres == res.relres and res2.lvalue == res.lvalue


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5], CASES[8], CASES[11]], ids=lambda c: c[0])
@pytest.mark.parametrize("tol", [1e-5, 1e-10])
def test_pcg_against_host_driven_cg(eng, case, tol):
    """The same iteration driven from the host reaches the same x.  The two runs do the same arithmetic with sums in
    different orders: after the same number of iterations they differ by rounding alone, 10 kappa eps |x|; when one
    of them takes one iteration more (its |r| sat on the threshold), that last step moves x by no more than the
    stopping rule resolves, tol |x| on top.  A case that misses this gets another seed, not a wider bound."""
    name, dims, cplx, twolayer, masked, precond = case
    p = Problem(eng, 31, dims, cplx, twolayer, masked)
    b, x0 = p.rhs(7)
    res, dx, _, _ = p.solve(b, x0, tol, precond)
    xh, kh = host_driven_cg(p, b, x0, tol, precond, 10 * p.n)
    x = dx.to_host().ravel()
    dev = np.linalg.norm(x - xh) / np.linalg.norm(x)
    print(f"{name} tol={tol:g}: iters device {res.iters} host {kh}, |x - x_host| / |x| = {dev:.3e}")
    assert res.status == 0
    assert abs(res.iters - kh) <= 1
    assert dev <= 10 * p.kappa * EPS + (tol if res.iters != kh else 0.0)


def test_pcg_zero_rhs(eng):
    p = Problem(eng, 41, ONE_SMALL, False, False, True)
    b, x0 = p.rhs(1)
    # b lives outside the masked space only: it vanishes under the mask
    b = (_rand(np.random.default_rng(2), p.shape, False) * ~p.mask).ravel()
    res, dx, _, st = p.solve(b, x0, 1e-8)
    assert res.status == 0 and res.iters == 0 and res.relres == 0.0 and res.lvalue == 0.0
    assert np.all(dx.to_host() == 0)
    assert st["end_tol"] == 1


@pytest.mark.parametrize("twolayer", [False, True])
def test_pcg_max_iter_one(eng, twolayer):
    """MPSE_ERR_NOCONV with the first iterate in x and the outputs filled: from x0 = 0, x1 = alpha z0 with z0 = b / diag,
    alpha = (b^H z0) / (z0^H A z0)."""
    p = Problem(eng, 51, ONE_SMALL, False, twolayer, False)
    b, _ = p.rhs(3)
    res, dx, db, st = p.solve(b, np.zeros_like(b), 1e-10, precond=True, max_iter=1)
    z0 = b / p.diag()
    alpha = np.vdot(b, z0).real / np.vdot(z0, p.apply(z0)).real
    x1 = alpha * z0
    x = dx.to_host().ravel()
    assert res.status == E.MPSE_ERR_NOCONV and res.iters == 1
    assert st["end_max_iter"] == 1 and st["matvecs"] == 1
    assert np.linalg.norm(x - x1) <= 1e-12 * np.linalg.norm(x1)
    r1 = np.linalg.norm(b - p.apply(x1)) / np.linalg.norm(b)
    assert r1 > 1e-10 and abs(res.relres - r1) <= 1e-10 * r1 + 1e-13
    direct = np.vdot(x1, p.apply(x1)).real - 2 * np.vdot(b, x1).real
    assert abs(res.lvalue - direct) <= 1e-12 * (abs(np.vdot(x1, p.apply(x1)).real) + abs(np.vdot(b, x1).real))


def test_pcg_indefinite_operator_returns(eng):
    """A shift below -lam_max makes the operator negative definite: the first curvature p^H A p is negative, the solve
    ends with MPSE_ERR_ARG and x is left at the (masked) start vector."""
    p = Problem(eng, 61, ONE_SMALL, False, False, False)
    lam, _ = p.k.spectrum()
    b, x0 = p.rhs(4)
    res, dx, _, st = p.solve(b, x0, 1e-8, check=False, shift=-(lam[-1] + 1.0))
    assert res.status == E.MPSE_ERR_ARG and res.iters == 0
    assert st["end_curvature"] == 1
    assert b"curvature" in eng.lib.mpse_last_error(eng.ctx)
    assert np.array_equal(dx.to_host().ravel(), x0)
    with pytest.raises(E.EngineError):
        p.solve(b, x0, 1e-8, shift=-(lam[-1] + 1.0))


def test_pcg_indefinite_operator_after_one_iteration(eng):
    """An indefinite operator whose curvature turns negative at the second step: shift = -(lam_min + lam_max) / 2 gives
    A the eigenvalues -h and +h on the lowest and the highest eigenvector of H, and b = u_max + 0.3 u_min spans an
    invariant plane on which the form x^H A x has signature (+, -).  From x0 = 0 without preconditioner p0 = b has the
    curvature h (1 - 0.09) > 0; p1 is A-conjugate to p0 inside that plane, so by the law of inertia its curvature is
    negative.  The solve ends there with MPSE_ERR_ARG, iters = 1 and x the iterate before that step,
    x1 = (b^H b / b^H A b) b."""
    p = Problem(eng, 62, ONE_SMALL, False, False, False)
    lam, idx = p.lam_h, p.lam_idx
    shift = -0.5 * (lam[0] + lam[-1])
    h = 0.5 * (lam[-1] - lam[0])
    b = (p.k.vector(idx[-1]) + 0.3 * p.k.vector(idx[0])).astype(np.float64)
    ab = p.k.apply(b) + shift * b
    assert np.vdot(b, ab) > 0.9 * h * 0.9
    x1 = np.vdot(b, b) / np.vdot(b, ab) * b
    res, dx, _, st = p.solve(b, np.zeros_like(b), 1e-12, check=False, shift=shift)
    x = dx.to_host().ravel()
    print(f"indefinite after one step: status {res.status} iters {res.iters} relres {res.relres:.3e}")
    assert res.status == E.MPSE_ERR_ARG and res.iters == 1
    assert st["end_curvature"] == 1 and st["solves"] == 1 and st["iterations"] == 1
    assert b"curvature" in eng.lib.mpse_last_error(eng.ctx)
    assert np.linalg.norm(x - x1) <= 1e-12 * np.linalg.norm(x1)
    r1 = np.linalg.norm(b - (p.k.apply(x1) + shift * x1)) / np.linalg.norm(b)
    assert abs(res.relres - r1) <= 1e-10 * r1


def test_pcg_argument_checks(eng):
    p = Problem(eng, 71, ONE_SMALL, False, False, False)
    b, x0 = p.rhs(8)
    dx = eng.asdevice(x0.reshape(p.shape))
    s0 = eng.pcg_stats()
    # x aliasing b
    assert eng.pcg(p.hop, dx, dx, shift=p.shift, check=False).status == E.MPSE_ERR_ARG
    assert eng.pcg_stats() == s0
    # a preconditioner diagonal with an entry that is not positive
    d = p.diag()
    d[17] = 0.0
    db = eng.asdevice(b.reshape(p.shape))
    res = eng.pcg(p.hop, db, dx, diag=eng.asdevice(d.reshape(p.shape)), shift=p.shift, check=False)
    assert res.status == E.MPSE_ERR_ARG and res.iters == 0
    assert np.array_equal(dx.to_host().ravel(), x0)
    # complex operator parts with real vectors
    pc = Problem(eng, 72, ONE_SMALL, True, False, False)
    assert eng.pcg(pc.hop, db, dx, shift=pc.shift, check=False).status == E.MPSE_ERR_ARG
