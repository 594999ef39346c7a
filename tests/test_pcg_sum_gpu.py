"""mpse_pcg_sum (Engine.pcg_sum): conjugate gradients over a weighted sum of two-layer terms on a centre with two physical
legs, on problems whose solution is known exactly.  T = A + B with A = (a0 F0 - omega) + F1[up leg] + a3 F3 and
B = (1 - a0) F0 + F2[down leg] + (1 - a3) F3 is a Kronecker sum of the four factors of a tests/kron_problems.py centre
(Dl, d_up, d_down, Dr); A and B commute, so (T - omega)^2 = A A + 2 A B + B B: three terms with weights 1, 2, 1, the
first on the up leg twice, the second with one layer per leg, the third on the down leg twice - the shape of the
finite-temperature correction-vector system.  x* = ((T - omega)^2 + shift)^-1 b follows from the factor eigenvectors.

The bounds are those of tests/test_pcg_gpu.py, derived there: |r| / |b| <= tol (the stopping rule), the recomputed
residual <= 2 tol |b|, |x - x*| <= kappa tol |x*| with kappa known from the factor eigenvalues, lvalue to 1e-12 of the
sums it is made of."""
import numpy as np
import pytest

from renormalizer_amd import engine as E

from contract_refs import dense_ft              # (tests/contract_refs.py)
from kron_problems import _rand, kron_problem   # (tests/kron_problems.py)
from test_pcg_gpu import Problem, _charges, k_wait   # the exact-solution bookkeeping of the one-operator tests

pytestmark = pytest.mark.gpu

UP, DOWN = E.LEG_UP, E.LEG_DOWN
WEIGHTS = (1.0, 2.0, 1.0)


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def _sq(e1, e2):
    """two-layer environment (bond in, layer 1, layer 2, bond out) of the product of two one-layer operators given as
    (bra, channel, ket) environments; layer 1 (e1) acts first"""
    return np.einsum("xba,dcx->abcd", e1, e2)


class SumProblem:
    def __init__(self, eng, seed, dims, cplx, masked, eta=0.5, width=5.0, shift=None):
        assert len(dims) == 4
        self.eng = eng
        charges = _charges(dims) if masked else None
        spacing = [width / (len(dims) * n) * (1.0 + 0.07 * i) for i, n in enumerate(dims)] + [0.0]
        k = kron_problem(seed, dims, cplx, charges=charges, spacing=spacing)
        # spectrum, exact solve, host apply and exact diagonal of (T - omega)^2 + shift: the two-layer Problem on T
        self.p = p = Problem.from_kron(eng, k, cplx, twolayer=True, charges=charges, eta=eta, shift=shift)
        self.shape, self.n, self.cplx = k.shape, k.n, cplx
        Dl, du, dv, Dr = dims
        a0, a3 = 0.6, 0.3
        f0, f1, f2, f3 = k.f
        edt = complex if cplx else float

        def one_layer(fl, fsite, d, fr):
            l, r = np.zeros((Dl, 3, Dl), dtype=edt), np.zeros((Dr, 3, Dr), dtype=edt)
            w = np.zeros((3, d, d, 3))
            for ch in range(3):
                l[:, ch, :] = fl if ch == 0 else np.eye(Dl)
                w[ch, :, :, ch] = fsite.real if ch == 1 else np.eye(d)
                r[:, ch, :] = fr if ch == 2 else np.eye(Dr)
            return l, w, r

        la, wa, ra = one_layer(a0 * f0 - p.omega * np.eye(Dl), f1, du, a3 * f3)
        lb, wb, rb = one_layer((1 - a0) * f0, f2, dv, (1 - a3) * f3)
        dev = eng.asdevice
        self.keep = [dev(wa), dev(wb)]
        dwa, dwb = self.keep
        self.terms = []
        for (l1, r1, w1, leg1), (l2, r2, w2, leg2) in (((la, ra, dwa, UP), (la, ra, dwa, UP)),
                                                       ((la, ra, dwa, UP), (lb, rb, dwb, DOWN)),
                                                       ((lb, rb, dwb, DOWN), (lb, rb, dwb, DOWN))):
            L, R = dev(_sq(l1, l2)), dev(_sq(r1, r2))
            self.keep += [L, R]
            self.terms.append(eng.ft_term(w1, w2, leg1, leg2, 0, 1, self.shape, L, R))
        self.dmask = p.dmask
        self.dtype = p.dtype

    def device_diag(self):
        eng = self.eng
        return eng.diag_ft_sum(self.terms, [eng.site_factor_ft(t) for t in self.terms], WEIGHTS, self.p.shift)

    def solve(self, b, x0, tol, precond=False, max_iter=0, check=True, shift=None):
        eng = self.eng
        db, dx = eng.asdevice(b.reshape(self.shape)), eng.asdevice(x0.reshape(self.shape))
        dd = self.device_diag() if precond else None
        s0, t0 = eng.pcg_stats(), eng.pcg_sum_stats()
        res = eng.pcg_sum(self.terms, WEIGHTS, db, dx, diag=dd, mask=self.dmask,
                          shift=self.p.shift if shift is None else shift, tol=tol, max_iter=max_iter, check=check)
        s1, t1 = eng.pcg_stats(), eng.pcg_sum_stats()
        st = {key: s1[key] - s0[key] for key in s1}
        st.update({"sum_" + key: t1[key] - t0[key] for key in t1})
        return res, dx, db, st

    def device_residual(self, dx, db):
        """|b - A x| from the term applications, mpse_mul_real and mpse_axpy, outside the solver"""
        eng = self.eng
        y = None
        for t, w in zip(self.terms, WEIGHTS):
            yt = eng.heff_apply_ft(t, dx)
            if y is None:
                y = yt.scale_(w)
            else:
                eng._check(eng.lib.mpse_axpy(eng.ctx, y.code, y.ptr, yt.ptr, y.size, w, 0.0))
        if self.dmask is not None:
            eng._check(eng.lib.mpse_mul_real(eng.ctx, y.code, y.ptr, self.dmask.ptr, y.size))
        eng._check(eng.lib.mpse_axpy(eng.ctx, y.code, y.ptr, dx.ptr, y.size, self.p.shift, 0.0))
        r = db.copy()
        eng._check(eng.lib.mpse_axpy(eng.ctx, r.code, r.ptr, y.ptr, r.size, -1.0, 0.0))
        return r.norm()


SMALL, MID = (9, 5, 6, 13), (24, 8, 7, 24)      # 3510 and 32256 elements; extents all different
CASES = [
    # (name, dims, complex, mask, preconditioner)
    ("small_f64", SMALL, False, False, False),
    ("small_f64_mask_pre", SMALL, False, True, True),
    ("small_c128_pre", SMALL, True, False, True),
    ("small_c128_mask", SMALL, True, True, False),
    ("mid_f64_pre", MID, False, False, True),
    ("mid_c128_mask_pre", MID, True, True, True),
]


def test_terms_sum_to_the_square(eng):
    """the three terms, weights 1, 2, 1, are (T - omega)^2 of the Kronecker sum; the device diagonal is its diagonal"""
    for cplx in (False, True):
        sp = SumProblem(eng, 5, SMALL, cplx, False)
        x = _rand(np.random.default_rng(1), sp.shape, cplx).astype(sp.dtype)
        dx = eng.asdevice(x)
        y = sum(w * eng.heff_apply_ft(t, dx).to_host() for t, w in zip(sp.terms, WEIGHTS))
        ref = sp.p.f_of_h(x.ravel()).reshape(sp.shape)
        assert np.abs(y - ref).max() <= 1e-11 * np.abs(ref).max()
        d = sp.device_diag().to_host().ravel()
        dref = sp.p.diag()
        assert np.abs(d - dref).max() <= 1e-12 * np.abs(dref).max()


@pytest.mark.parametrize("tol", [1e-5, 1e-10])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pcg_sum_exact_solution(eng, case, tol):
    name, dims, cplx, masked, precond = case
    sp = SumProblem(eng, 11, dims, cplx, masked)
    p = sp.p
    assert p.lam_a.min() > 0
    b, x0 = p.rhs(5)
    xs = p.exact(b)
    res, dx, db, st = sp.solve(b, x0, tol, precond)
    x = dx.to_host().ravel()
    nb = np.linalg.norm(b)
    true_res = sp.device_residual(dx, db)
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
    assert st["twolayer"] == 0 and st["masked"] == int(masked)
    assert 0 <= st["matvecs"] - st["iterations"] <= k_wait(eng) - 1
    assert st["sum_solves"] == 1 and st["sum_iterations"] == res.iters
    assert st["sum_term_applies"] == 3 * st["matvecs"] and st["sum_host_waits"] == st["host_waits"]
    # the host read the control block on the K schedule and nothing else: waits = ceil((iters + 1) / K)
    K = k_wait(eng)
    assert st["host_waits"] == res.iters // K + 1


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[5]], ids=lambda c: c[0])
def test_pcg_sum_decision_on_device(eng, case):
    """x is final at the deciding iteration: a second solve limited to the reported iteration count returns x bit for
    bit - the products of all three terms past the decision returned at once."""
    name, dims, cplx, masked, precond = case
    sp = SumProblem(eng, 21, dims, cplx, masked)
    b, x0 = sp.p.rhs(6)
    res, dx, _, st = sp.solve(b, x0, 1e-8, precond)
    assert res.status == 0 and res.iters > 0
    assert st["matvecs"] - st["iterations"] <= k_wait(eng) - 1
    res2, dx2, _, st2 = sp.solve(b, x0, 1e-8, precond, max_iter=res.iters)
    assert res2.status == 0 and res2.iters == res.iters
    assert st2["matvecs"] == res.iters
    assert np.array_equal(dx.to_host(), dx2.to_host())
    assert res2.relres == res.relres and res2.lvalue == res.lvalue


def test_pcg_sum_negative_curvature(eng):
    """a shift below -lam_max((T - omega)^2): negative definite, the first curvature ends the solve with MPSE_ERR_ARG
    and x stays the start vector"""
    sp = SumProblem(eng, 61, SMALL, False, False)
    p = sp.p
    b, x0 = p.rhs(4)
    bad = -(((p.lam_h - p.omega) ** 2).max() + 1.0)
    res, dx, _, st = sp.solve(b, x0, 1e-8, check=False, shift=bad)
    assert res.status == E.MPSE_ERR_ARG and res.iters == 0
    assert st["end_curvature"] == 1
    assert b"curvature" in eng.lib.mpse_last_error(eng.ctx)
    assert np.array_equal(dx.to_host().ravel(), x0)
    with pytest.raises(E.EngineError):
        sp.solve(b, x0, 1e-8, shift=bad)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_one_term_is_the_two_layer_solve(eng, cplx, masked):
    """one term, weight 1, both layers on the up leg with one MPO site and d_down = 1: the bits of mpse_pcg(twolayer=1)"""
    p = Problem(eng, 31, (23, 11, 29), cplx, True, masked)
    b, x0 = p.rhs(7)
    res, dx, _, _ = p.solve(b, x0, 1e-8, precond=True)
    hop = p.hop
    Dl, d, Dr = p.shape
    term = eng.ft_term(hop.cmo[0], hop.cmo[0], UP, UP, 1, 1, (Dl, d, 1, Dr), hop.l, hop.r)
    db, dx2 = eng.asdevice(b.reshape(Dl, d, 1, Dr)), eng.asdevice(x0.reshape(Dl, d, 1, Dr))
    dd = eng.asdevice(p.diag().reshape(Dl, d, 1, Dr))
    res2 = eng.pcg_sum([term], [1.0], db, dx2, diag=dd, mask=p.dmask, shift=p.shift, tol=1e-8)
    assert res.status == 0 and res2.status == 0
    assert res2.iters == res.iters and res2.relres == res.relres and res2.lvalue == res.lvalue
    assert np.array_equal(dx.to_host().ravel(), dx2.to_host().ravel())


def test_pcg_sum_argument_checks(eng):
    sp = SumProblem(eng, 71, SMALL, False, False)
    b, x0 = sp.p.rhs(8)
    dx = eng.asdevice(x0.reshape(sp.shape))
    s0 = eng.pcg_stats()
    assert eng.pcg_sum(sp.terms, WEIGHTS, dx, dx, shift=sp.p.shift, check=False).status == E.MPSE_ERR_ARG
    db = eng.asdevice(b.reshape(sp.shape))
    assert eng.pcg_sum(sp.terms * 2, WEIGHTS * 2, db, dx, shift=sp.p.shift, check=False).status == E.MPSE_ERR_ARG
    assert eng.pcg_stats() == s0
    # the down leg first, the up leg second: refused (environments of the matching shape: all bonds are 3 here)
    wa, wb, L, R = sp.keep[0], sp.keep[1], sp.keep[4], sp.keep[5]
    assert L.shape == (sp.shape[0], wb.shape[0], wa.shape[0], sp.shape[0])
    swapped = eng.ft_term(wb, wa, DOWN, UP, 0, 0, sp.shape, L, R)
    with pytest.raises(ValueError):
        eng.pcg_sum([swapped], [1.0], db, dx, shift=sp.p.shift)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("trans", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("legs", [(UP, UP), (UP, DOWN), (DOWN, DOWN)], ids=["M1", "M2", "M3"])
def test_device_diagonal_of_a_term(eng, legs, trans, cplx):
    """mpse_site_factor_ft / mpse_diag_ft against the diagonal of the dense projected term (the term applied to every
    unit vector), with MPO sites that are NOT symmetric and unequal bonds, so that a wrong transposition flag or a
    swapped bond changes it.  Hermitian environments are not needed: the diagonal is compared as Re(diag)."""
    rng = np.random.default_rng(23)
    Dl, du, dv, Dr = 3, 2, 3, 4
    wl1, wr1, wl2, wr2 = 2, 3, 4, 2
    d1 = du if legs[0] == UP else dv
    d2 = du if legs[1] == UP else dv
    dev = eng.asdevice
    hw1, hw2 = rng.standard_normal((wl1, d1, d1, wr1)), rng.standard_normal((wl2, d2, d2, wr2))
    hl, hr = _rand(rng, (Dl, wl1, wl2, Dl), cplx), _rand(rng, (Dr, wr1, wr2, Dr), cplx)
    w1, w2, L, R = dev(hw1), dev(hw2), dev(hl), dev(hr)
    shape = (Dl, du, dv, Dr)
    term = eng.ft_term(w1, w2, legs[0], legs[1], trans[0], trans[1], shape, L, R)
    n = int(np.prod(shape))
    dense = np.empty((n, n), dtype=complex if cplx else float)
    for k in range(n):
        e = np.zeros(n, dtype=dense.dtype)
        e[k] = 1.0
        dense[:, k] = eng.heff_apply_ft(term, dev(e.reshape(shape))).to_host().ravel()
    # the dense operator is built with mpse_heff_apply_ft, itself code under test: anchored to the NumPy statement of
    # the term (tests/contract_refs.py), so that a convention error shared by the matvec and the diagonal does not pass
    dense_np = dense_ft(hl, hr, hw1, hw2, legs, trans, shape)
    assert np.abs(dense - dense_np).max() <= 1e-12 * np.abs(dense_np).max()
    ref = np.real(np.diag(dense))
    fac = eng.site_factor_ft(term)
    d = eng.diag_ft_sum([term], [fac], [1.0], 0.0).to_host().ravel()
    assert np.abs(d - ref).max() <= 1e-12 * np.abs(ref).max()
    d2w = eng.diag_ft_sum([term, term], [fac, fac], [0.5, 2.0], 0.75).to_host().ravel()
    assert np.abs(d2w - (0.75 + 2.5 * ref)).max() <= 1e-12 * (0.75 + 2.5 * np.abs(ref).max())
