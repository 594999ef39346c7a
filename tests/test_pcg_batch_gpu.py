"""The batched conjugate gradients of the engine (mpse_pcg_batch, through Engine.pcg_batch) on two-layer centre problems
(H - omega)^2 + shift whose solution is known exactly (tests/kron_problems.py, the ``Problem`` of test_pcg_gpu.py).

The Kron centres have three MPO channels; wider MPO bonds are made by padding: further channels of L hold random numbers
and meet only zero rows of W, further right channels of W hold random numbers and meet only zero channels of R - the
operator is unchanged, every index of the kernel is exercised with non-trivial data.

Bounds (those of test_pcg_gpu.py, none taken from the solver): returned |r| / |b| <= tol; |b - A x| recomputed on the
host <= 2 tol |b|; |x - x*| <= kappa tol |x*| with kappa exact from the factor eigenvalues; lvalue against
Re(x^H A x) - 2 Re(b^H x) of the returned x to 1e-12 of the summed magnitudes.  Composition independence is bitwise."""
import numpy as np
import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.cv.lockstep import (SM2_BMAX, SM2_DMAX, SM2_LDS_MAX, SM2_WMAX, small2_eligible)
from renormalizer_amd.mps.hop_expr import hop_expr

from kron_problems import _rand
from test_pcg_gpu import Problem, _square_env

pytestmark = pytest.mark.gpu

TOL = 1e-8
OK, NOCONV, ARG = 0, 3, 5


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def _pad(rng, k, l1, w):
    """one-layer L, R and MPO site of the Kron centre ``k`` widened to ``w`` channels without changing the operator"""
    nf = l1.shape[1]
    Dl, d, Dr = k.shape
    cplx = np.iscomplexobj(l1)
    L = np.zeros((Dl, w, Dl), dtype=l1.dtype)
    R = np.zeros((Dr, w, Dr), dtype=k.r.dtype)
    W = np.zeros((w, d, d, w))
    L[:, :nf, :], R[:, :nf, :], W[:nf, :, :, :nf] = l1, k.r, k.cmo[0]
    if w > nf:
        L[:, nf:, :] = _rand(rng, (Dl, w - nf, Dl), cplx)
        W[:nf, :, :, nf:] = rng.standard_normal((nf, d, d, w - nf))
    return L, R, W


class Member:
    """One system of a batch: a two-layer ``Problem`` with its own omega, shift, MPO bond, right-hand side and start."""

    def __init__(self, eng, seed, dims, w, cplx, masked, domega=0.01, shift=None, rhs_seed=None):
        p = Problem(eng, seed, dims, cplx, True, masked, shift=shift)
        lam = p.lam_h
        p.omega = 0.5 * (lam[0] + lam[-1]) + domega
        p.lam_a = (lam - p.omega) ** 2 + p.shift
        p.kappa = p.lam_a.max() / p.lam_a.min()
        k = p.k
        l1 = k.l.copy()
        l1[:, 0, :] -= p.omega * np.eye(dims[0])
        L, R, W = _pad(np.random.default_rng(seed + 977), k, l1, w)
        p.hop = hop_expr(eng.asdevice(_square_env(L)), eng.asdevice(_square_env(R)), [eng.asdevice(W)], k.shape, True)
        self.p, self.eng, self.w, self.dims, self.cplx = p, eng, w, dims, cplx
        self.b, self.x0 = p.rhs(seed + 31 if rhs_seed is None else rhs_seed)
        self.diag = p.diag()
        self.eligible = small2_eligible(dims[0], dims[1], dims[2], w, w, cplx)

    def device(self, precond=True):
        eng, p = self.eng, self.p
        db, dx = eng.asdevice(self.b.reshape(p.shape)), eng.asdevice(self.x0.reshape(p.shape))
        dd = eng.asdevice(self.diag.reshape(p.shape)) if precond else None
        return db, dx, dd

    def check(self, res, x, tol=TOL):
        p, b = self.p, self.b
        assert res.status == OK
        nb = np.linalg.norm(b)
        xs = p.exact(b)
        ax = p.apply(x)
        true_res = np.linalg.norm(b - ax)
        err = np.linalg.norm(x - xs)
        xax, bx = np.vdot(x, ax).real, np.vdot(b, x).real
        print(f"{self.dims} w={self.w} cplx={self.cplx}: iters {res.iters} relres {res.relres:.2e} true "
              f"{true_res / nb:.2e} err {err / np.linalg.norm(xs):.2e} (kappa {p.kappa:.1f})")
        assert res.relres <= tol
        assert true_res <= 2 * tol * nb
        assert err <= p.kappa * tol * np.linalg.norm(xs)
        assert abs(res.lvalue - (xax - 2 * bx)) <= 1e-12 * (abs(xax) + abs(bx))


def solve(eng, members, tol=TOL, max_iter=0, precond=True, diags=None):
    dev = [m.device(precond) for m in members]
    if diags is None:
        diags = [d[2] for d in dev]
    s0 = eng.pcg_batch_stats()
    res = eng.pcg_batch([m.p.hop for m in members], [d[0] for d in dev], [d[1] for d in dev], diags,
                        [m.p.dmask for m in members], [m.p.shift for m in members], tol, max_iter)
    s1 = eng.pcg_batch_stats()
    return res, [d[1].to_host().ravel() for d in dev], {k: s1[k] - s0[k] for k in s1}


def _lds_edge():
    """largest Dl at the widest MPO bond and physical dimension that the LDS budget admits for a complex centre (a
    real one fits at every bond dimension), from the rule"""
    Dl = max(v for v in range(1, SM2_BMAX + 1) if small2_eligible(v, SM2_DMAX, 4, SM2_WMAX, SM2_WMAX, True))
    assert Dl < SM2_BMAX and not small2_eligible(Dl + 1, SM2_DMAX, 4, SM2_WMAX, SM2_WMAX, True)
    return Dl


# (dims, w, expected eligibility of the real form): the issue's shapes, one at each limit of the rule and one outside
SHAPES = [((5, 3, 7), 3, True), ((17, 4, 33), 5, True), ((24, 16, 24), 5, True),
          ((6, 3, 5), SM2_WMAX, True), ((6, 3, 5), SM2_WMAX + 1, False),
          ((5, SM2_DMAX + 1, 4), 3, False),
          ((SM2_BMAX, 2, 5), 3, True), ((SM2_BMAX + 1, 2, 5), 3, False), ((5, 2, SM2_BMAX + 1), 3, False),
          ((_lds_edge(), SM2_DMAX, 4), SM2_WMAX, True), ((_lds_edge() + 1, SM2_DMAX, 4), SM2_WMAX, True)]


def test_rule_matches_engine(eng):
    """the Python statement of the eligibility rule is the engine's"""
    info = (E.C.c_int64 * 8)()
    for dims, w, real_ok in SHAPES:
        for cplx in (False, True):
            code = E.dtype_code(np.dtype(np.complex128 if cplx else np.float64))
            got = eng.lib.mpse_pcg_batch_plan(code, dims[0], dims[1], dims[2], w, w, info, 8)
            assert bool(got) == small2_eligible(dims[0], dims[1], dims[2], w, w, cplx), (dims, w, cplx)
            assert list(info[:4]) == [SM2_WMAX, SM2_DMAX, SM2_BMAX, SM2_LDS_MAX]
            assert (info[4] > 0) == bool(got) and info[4] <= SM2_LDS_MAX
        assert small2_eligible(dims[0], dims[1], dims[2], w, w, False) == real_ok, (dims, w)


@pytest.mark.parametrize("cplx", (False, True), ids=("real", "complex"))
@pytest.mark.parametrize("masked", (False, True), ids=("full", "masked"))
@pytest.mark.parametrize("dims,w,real_ok", SHAPES, ids=[f"{d[0]}x{d[1]}x{d[2]}w{w}" for d, w, _ in SHAPES])
def test_exact_every_member(eng, dims, w, real_ok, masked, cplx):
    """three members per shape with different omega, right-hand side and shift, on the path their shape selects"""
    members = [Member(eng, 100 + 7 * i, dims, w, cplx, masked, domega=0.01 + 0.13 * i, shift=0.25 + 0.2 * i)
               for i in range(3)]
    res, xs, st = solve(eng, members)
    for m, r, x in zip(members, res, xs):
        m.check(r, x)
    elig = members[0].eligible
    assert st["batched_members"] == (3 if elig else 0) and st["single_members"] == (0 if elig else 3)
    if elig:
        # one matvec launch per iteration of the launch set, not one per member
        k = eng.pcg_stats()["wait_interval"]
        most = max(r.iters for r in res)
        assert st["launch_sets"] == 1
        assert most <= st["matvec_launches"] <= most + k - 1
        assert st["matvec_launches"] < sum(r.iters for r in res)


def test_handed_to_pcg_bitwise(eng):
    """a shape outside the rule, a one-layer member and a two-site member run as mpse_pcg runs them: bitwise Engine.pcg,
    and every counter of ``pcg_stats`` moves as it does over that call"""
    moved = lambda a, b: {k: b[k] - a[k] for k in b if k != "wait_interval"}       # (wait_interval is no count)
    outside = Member(eng, 5, (5, SM2_DMAX + 1, 4), 3, False, True)
    cases = [(outside.p, outside.b, outside.x0, outside.diag)]
    for dims, two in (((9, 5, 11), False), ((6, 3, 4, 5), True)):
        p = Problem(eng, 11, dims, False, two, True)
        b, x0 = p.rhs(3)
        cases.append((p, b, x0, p.diag()))
    for p, b, x0, dg in cases:
        dev = lambda: (eng.asdevice(b.reshape(p.shape)), eng.asdevice(x0.reshape(p.shape)),
                       eng.asdevice(dg.reshape(p.shape)))
        db, dx, dd = dev()
        c0 = eng.pcg_stats()
        one = eng.pcg(p.hop, db, dx, diag=dd, mask=p.dmask, shift=p.shift, tol=TOL)
        c1 = eng.pcg_stats()
        db2, dx2, dd2 = dev()
        s0 = eng.pcg_batch_stats()
        got = eng.pcg_batch([p.hop], [db2], [dx2], [dd2], [p.dmask], [p.shift], TOL)[0]
        s1 = eng.pcg_batch_stats()
        c2 = eng.pcg_stats()
        assert s1["single_members"] - s0["single_members"] == 1 and s1["batched_members"] == s0["batched_members"]
        assert moved(c1, c2) == moved(c0, c1) and moved(c0, c1)["solves"] == 1
        assert tuple(got) == tuple(one) and one.status == OK
        assert np.array_equal(dx.to_host(), dx2.to_host())


def test_composition_independence(eng):
    """the same member alone, first / middle / last of five, and on either side of a launch-set boundary: same bits"""
    dims, w = (5, 3, 7), 3
    limit = eng.pcg_batch_stats()["set_limit"]
    me = Member(eng, 41, dims, w, True, True, domega=0.07)
    others = [Member(eng, 300 + i, dims, w, True, True, domega=0.02 * i, shift=0.25 + 0.05 * i) for i in range(4)]
    res, xs, st = solve(eng, [me])
    assert st["batched_members"] == 1 and st["launch_sets"] == 1
    me.check(res[0], xs[0])
    ref_r, ref_x = res[0], xs[0]
    for pos in (0, 2, 4):
        batch = others[:pos] + [me] + others[pos:]
        res, xs, st = solve(eng, batch)
        assert st["batched_members"] == 5 and st["launch_sets"] == 1
        assert tuple(res[pos]) == tuple(ref_r) and np.array_equal(xs[pos], ref_x), pos
    fill = [others[i % 4] for i in range(limit)]
    for pos in (0, limit):           # last of the full set's neighbours / alone in the second set
        batch = fill[:pos] + [me] + fill[pos:]
        res, xs, st = solve(eng, batch)
        assert st["batched_members"] == limit + 1 and st["launch_sets"] == 2
        assert tuple(res[pos]) == tuple(ref_r) and np.array_equal(xs[pos], ref_x), pos
        assert tuple(res[(pos + 1) % (limit + 1)]) == tuple(solve(eng, [batch[(pos + 1) % (limit + 1)]])[0][0])


def test_members_that_end_differently(eng):
    dims, w, cplx = (17, 4, 33), 5, False
    # shift 200 on a spectrum of (H - omega)^2 within [0, 6.5]: kappa < 1.04, three iterations reach 1e-5
    healthy = Member(eng, 61, dims, w, cplx, True, shift=200.0)
    zero_b = Member(eng, 62, dims, w, cplx, True)
    zero_b.b = (_rand(np.random.default_rng(1), dims, cplx) * (1 - zero_b.p.mask)).ravel()
    slow = Member(eng, 63, dims, w, cplx, True, shift=1e-4)         # kappa of the order 1e4
    bad = Member(eng, 64, dims, w, cplx, True)
    bad.diag = bad.diag.copy()
    bad.diag[bad.diag.size // 2] = -1.0
    tol = 1e-5
    res, xs, st = solve(eng, [healthy, zero_b, slow, bad], tol=tol, max_iter=3)      # (the call itself returns 0)
    assert st["batched_members"] == 4 and st["launch_sets"] == 1
    healthy.check(res[0], xs[0], tol=tol)
    assert 1 <= res[0].iters <= 3
    assert res[1].status == OK and res[1].iters == 0 and not xs[1].any()
    assert res[2].status == NOCONV and res[2].iters == 3 and res[2].relres > tol and np.isfinite(res[2].lvalue)
    assert np.isfinite(xs[2]).all() and not np.array_equal(xs[2], slow.x0)
    assert res[3].status == ARG
    alone, xa, _ = solve(eng, [healthy], tol=tol, max_iter=3)
    assert tuple(alone[0]) == tuple(res[0]) and np.array_equal(xa[0], xs[0])


def test_mixed_batch(eng):
    """two shapes interleaved plus one member outside the rule: two launch sets and one single solve"""
    a = [Member(eng, 70 + i, (5, 3, 7), 3, False, True, domega=0.1 * i) for i in range(2)]
    b = [Member(eng, 80 + i, (17, 4, 33), 5, False, False, domega=0.1 * i) for i in range(2)]
    out = Member(eng, 90, (5, SM2_DMAX + 1, 4), 3, False, True)
    batch = [a[0], b[0], out, a[1], b[1]]
    res, xs, st = solve(eng, batch)
    for m, r, x in zip(batch, res, xs):
        m.check(r, x)
    assert st["launch_sets"] == 2 and st["batched_members"] == 4 and st["single_members"] == 1
