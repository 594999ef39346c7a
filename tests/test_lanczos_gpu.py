"""mpse_expm_lanczos (mpse_lanczos.hip) against exact exponentials, on every path of the solve.

The operators are Kronecker sums (tests/kron_problems.py): exp(dt H) C is exact in float64 from the eigendecompositions
of the small factors, at any centre size.  Each case asserts the deltas of ``mpse_expm_lanczos_path_stats`` for the
path it is named for, so a threshold that moves cannot take a case off its path silently.

  * exact by breakdown: C spans k <= 8 exact eigenvectors, the solve must stop at k vectors (rtol = 1e-14, atol = 0) and
    give sum_i exp(dt l_i) c_i u_i to 20 eps (k + 2^s), s the scaling exponent of the on-device exponential
    (lz_coefs: rho = |dt| x Gershgorin bound of T_k, 2^s repetitions of a Taylor series at rho / 2^s <= 2);
  * every scaling band of lz_coefs, (0, 1/2], (1/2, 1], (1, 2], (2^s, 2^(s+1)] for s = 1..8 and above 512 (the host),
    with real-time, imaginary-time (both signs) and complex steps; rho is placed mid-band from a host Lanczos of the
    same problem (the operator is shifted by E0 for the upper bands);
  * the hand-overs of the asynchronous solve (need_host at a later check, the 64-vector limit, max_dim), the matvec
    paths the solve drives, the run-ahead hint, batched solves, out == C, scaling of C by powers of two and bad
    start vectors.
"""
import ctypes as C
import math

import numpy as np
import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.mps.hop_expr import centre_tile_mask, hop_expr

from kron_problems import _rand, kron_problem   # (tests/kron_problems.py)

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


# ----------------------------------------------------------------------------------------------- helpers

def _delta(a, b):
    return {k: b[k] - a[k] for k in a if b[k] != a[k]}


def _hop(k):
    return hop_expr(k.l, k.r, k.cmo, k.shape)


def _solve(eng, hop, c, dt, rtol, atol=0.0, max_dim=0, out=None):
    """mpse_expm_lanczos on device vector c: (status, result on the host, nvec, counter deltas)"""
    dt = complex(dt)
    if out is None:
        out = eng.empty(c.shape, c.dtype)
    nv = C.c_int()
    s0 = eng.lanczos_path_stats()
    if getattr(hop, "cmask", None) is not None:
        eng._check(eng.lib.mpse_expm_centre_mask(eng.ctx, hop.cmask.ptr, hop.cmask.nbytes))
    st = eng.lib.mpse_expm_lanczos(eng.ctx, c.code, C.byref(hop.heff), dt.real, dt.imag, c.ptr, out.ptr, rtol, atol,
                                   max_dim, C.byref(nv))
    return st, out.to_host().ravel(), nv.value, _delta(s0, eng.lanczos_path_stats())


def _batch(eng, hops, cs, dt, rtol, atol=0.0, outs=None):
    dt = complex(dt)
    if outs is None:
        outs = [eng.empty(c.shape, c.dtype) for c in cs]
    cnt = len(hops)
    harr = (type(hops[0].heff) * cnt)(*[h.heff for h in hops])
    carr = (C.c_void_p * cnt)(*[c.ptr for c in cs])
    oarr = (C.c_void_p * cnt)(*[o.ptr for o in outs])
    nv = (C.c_int * cnt)()
    s0, b0 = eng.lanczos_path_stats(), eng.lanczos_batch_stats()
    st = eng.lib.mpse_expm_lanczos_batch(eng.ctx, cs[0].code, cnt, harr, dt.real, dt.imag, carr, oarr, rtol, atol, 0, nv)
    b1 = eng.lanczos_batch_stats()
    return (st, [o.to_host().ravel() for o in outs], list(nv), _delta(s0, eng.lanczos_path_stats()),
            (b1[0] - b0[0], b1[1] - b0[1]))


def _lanczos(apply, c, m):
    """host Lanczos (float64, the engine's recurrence): alpha, beta of up to m steps, stopping at a breakdown"""
    tiny = 100 * len(c) * EPS
    v = c / np.linalg.norm(c)
    vp, bprev = np.zeros_like(v), 0.0
    alpha, beta = [], []
    for _ in range(m):
        w = apply(v)
        a = np.vdot(v, w).real
        w = w - a * v - bprev * vp
        b = np.linalg.norm(w)
        alpha.append(a)
        if b < tiny:
            break
        beta.append(b)
        vp, v, bprev = v, w / b, b
    return np.array(alpha), np.array(beta[:len(alpha) - 1])


def _gersh(alpha, beta):
    m = len(alpha)
    b = np.zeros(m + 1)
    b[1:m] = np.abs(beta[:m - 1])
    return float(np.max(np.abs(alpha) + b[:m] + b[1:]))


def _band(rho):
    s = 0
    while rho / 2.0 ** s > 2.0:
        s += 1
    return s


def _nrm(x):
    """2-norm without overflow (imaginary-time results reach 1e260)"""
    m = float(np.abs(x).max())
    return m * float(np.linalg.norm(x / m)) if m > 0 else 0.0


def _relerr(x, ref):
    return _nrm(x - ref) / _nrm(ref)


def _eig_start(k, kk, rng, cplx):
    """C = kk exact eigenvectors spread evenly over the spectrum with coefficients of modulus 1: (C, eigenvalues,
    coefs, vectors).  (Up to kk = 8 the engine's recurrence - no re-orthogonalisation - meets beta_(kk-1) < 100 n eps on
    these operators; for more vectors rounding leaves beta_(kk-1) above that threshold, see _lanczos.)"""
    vals, idx = k.spectrum()
    pick = np.unique(np.linspace(0, len(vals) - 1, kk).round().astype(int))
    U = np.stack([k.vector(idx[i]) for i in pick], axis=1)
    coef = np.exp(2j * np.pi * rng.uniform(size=kk)) if cplx else rng.choice([-1.0, 1.0], kk)
    c = U @ coef
    return (c if cplx else c.real), vals[pick], coef, U


def _exact_eig(dt, lam, coef, U):
    return U @ (np.exp(complex(dt) * lam) * coef)


SYNC_DIMS, ASYNC_DIMS = (5, 4, 6), (8, 5, 9)          # n = 120 (synchronous solve), 360 (asynchronous)


# =============================================================================================== 1. exact by breakdown

@pytest.mark.parametrize("cplx", [True, False], ids=["c128", "f64"])
@pytest.mark.parametrize("path", ["sync", "async"])
def test_exact_by_breakdown(eng, path, cplx):
    """k = 1..8 exact eigenvectors: the breakdown must end the solve at k vectors, before, at and after the merged
    first check (j = 6: k <= 7) and at the next one (j = 8), with the exact result to 20 eps (k + 1) (rho in (1/2, 1]:
    s = 0)."""
    k = kron_problem(11, SYNC_DIMS if path == "sync" else ASYNC_DIMS, cplx)
    hop = _hop(k)
    rng = np.random.default_rng(5)
    worst = 0.0
    for kk in range(1, 9):
        c, lam, coef, U = _eig_start(k, kk, rng, cplx)
        al, be = _lanczos(k.apply, c, 20)
        assert len(al) == kk
        tau = 0.7 / _gersh(al, be)
        dt = -1j * tau if cplx else tau
        st, out, nv, d = _solve(eng, hop, eng.asdevice(c), dt, 1e-14)
        assert st == 0 and nv == kk, (kk, st, nv, d)
        err = _relerr(out, _exact_eig(dt, lam, coef, U))
        worst = max(worst, err)
        assert err <= 20 * EPS * (kk + 1), (kk, err)
        if path == "sync":
            assert d.get("sync") == 1 and d.get("breakdown_sync") == 1 and "async_done" not in d, d
        else:
            assert d.get("async_done") == 1 and d.get("breakdown_async") == 1 and "sync" not in d, d
            assert d.get("host_waits", 0) >= 1
            if kk <= 7:
                assert d.get("merged_first") == 1, (kk, d)
    print(f"exact-by-breakdown {path} {'c128' if cplx else 'f64'}: worst relative error {worst:.2e}")


# =============================================================================================== 2. scaling bands

BANDS = [(-2, 0.0, 0.5), (-1, 0.5, 1.0), (0, 1.0, 2.0)] + [(s, 2.0 ** s, 2.0 ** (s + 1)) for s in range(1, 9)] + \
        [(9, 512.0, 1024.0)]
# (band, position): "mid" at the log midpoint, "top" at hi / 1.06 - x = rho / 2^s near 2, where every term of the longest
# series counts (a 19-term series leaves ~2e-14 per repetition there on a growing step, ~1.5e-13 on a real-time one)
BAND_CASES = [(b, "mid") for b in BANDS] + [(b, "top") for b in BANDS if b[0] < 9]
# kind: (dt / |dt|, sign of E0, decays).  imag_neg decays along the start vector (dt < 0, E0 > 0); the others grow or
# keep the norm
KINDS = {"real_time": (-1j, 1.0, False), "imag_pos": (1.0, 1.0, False), "imag_neg": (-1.0, 1.0, True),
         "complex": (0.6 - 0.8j, 1.0, False)}


def _band_problem(kind_dt, sign, band, pos, kk, cplx, seed=21):
    """(Kron, dt, C, lam, coef, U, s, x, breaks): kk exact eigenvectors, rho = |dt| g(T_kk) at ``pos`` in the band.
    Bands s <= 0: E0 = 0, |dt| = target / g.  Upper bands: |dt| g0 = 1/2 for the unshifted operator and the shift E0
    (of sign ``sign``) brings |dt| g(T_kk) to the target."""
    s, lo, hi = band
    if s == 9:
        target = 600.0
    else:
        target = np.sqrt(max(lo, 0.125) * hi) if pos == "mid" else hi / 1.06
    k0 = kron_problem(seed, ASYNC_DIMS, cplx)
    rng = np.random.default_rng(seed + kk)
    c, lam0, coef, U = _eig_start(k0, kk, rng, cplx)
    al, be = _lanczos(k0.apply, c, 20)
    assert len(al) == kk
    g0 = _gersh(al, be)
    if s <= 0:
        tau, e0 = target / g0, 0.0
    else:
        tau = 0.5 / g0
        b = np.zeros(len(al) + 1)
        b[1:len(al)] = np.abs(be)
        h = float(np.max(sign * al + b[:-1] + b[1:]))
        e0 = sign * (target / tau - h)
        assert abs(e0) >= np.abs(al).max()
    k = kron_problem(seed, ASYNC_DIMS, cplx, shift=e0)
    al2, be2 = _lanczos(k.apply, c, 20)
    rho = tau * _gersh(al2, be2)
    assert lo * 1.05 < rho < hi / 1.05 if s < 9 else rho > 1.05 * 512, (band, rho)
    assert _band(rho) == max(s, 0)
    # far from zero the shifted factor u diag(ev + E0) u^H holds rounding of order eps |E0|, above 100 n eps: then
    # beta_(kk-1) stays above the breakdown threshold and the solve stops by convergence, on the same Krylov space
    return k, kind_dt * tau, c, lam0 + e0, coef, U, max(s, 0), rho / 2.0 ** max(s, 0), len(al2) == kk


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("band,pos", BAND_CASES, ids=[f"s{b[0]}-{p}" for b, p in BAND_CASES])
def test_scaling_bands(eng, band, pos, kind):
    """exact by breakdown (or by convergence far from zero) to 20 eps (k + 2^s) on growing and real-time steps; a
    decaying step loses what the series cancels, a factor e^(2x) per repetition: 20 eps (k + 2^s e^(2x))"""
    dts, sign, decays = KINDS[kind]
    for cplx in ([True, False] if kind.startswith("imag") else [True]):
        kk = 4
        k, dt, c, lam, coef, U, s, x, breaks = _band_problem(dts, sign, band, pos, kk, cplx)
        hop = _hop(k)
        st, out, nv, d = _solve(eng, hop, eng.asdevice(c), dt, 1e-14)
        assert st == 0 and (nv == kk if breaks else nv <= 2 * kk), (st, nv, d)
        err = _relerr(out, _exact_eig(dt, lam, coef, U))
        bound = 20 * EPS * (kk + 2 ** s * (np.exp(2 * x) if decays else 1.0))
        assert err <= bound, (band, pos, kind, cplx, err, bound)
        end = ("breakdown_async" if band[0] < 9 else "breakdown_sync") if breaks else "converged"
        if band[0] < 9:
            assert d.get("async_done") == 1 and d.get(end) == 1 and "sync" not in d, d
        else:
            assert d.get("host_first") == 1 and d.get("sync") == 1 and d.get(end) == 1, d
        # a generic start vector on the same operator, rtol = 1e-10
        g = _rand(np.random.default_rng(3), (k.n,), cplx)
        st, out, nv, d = _solve(eng, hop, eng.asdevice(g), dt, 1e-10)
        assert st == 0, (st, d)
        ex = k.expm(dt, g)
        assert _nrm(out - ex) <= 10 * 1e-10 * _nrm(ex) + 1e-13 * _nrm(g), (band, kind)
        if band[0] < 9:
            assert d.get("async_done") == 1 and "sync" not in d, d
        else:
            assert d.get("host_first", 0) + d.get("host_later", 0) == 1 and d.get("sync") == 1, d


# =============================================================================================== 3. hand-overs

def _later_host_problem():
    """need_host at the second check the host reads: |dt| g(T_7) < 512 < |dt| g(T_9) (a narrow spectrum far from zero:
    the Krylov space converges in ~15 vectors while g grows with m).  Its centre size is used by no other solve of the
    context of its own, so no run-ahead hint of another solve moves the host's first wait from j = 6."""
    k = kron_problem(41, (8, 5, 11), True, shift=200.0, spacing=[0.05, 0.03, 0.04])
    c = _rand(np.random.default_rng(4), (k.n,), True)
    al, be = _lanczos(k.apply, c, 9)
    g7, g9 = _gersh(al[:7], be[:6]), _gersh(al[:9], be[:8])
    assert g9 > g7 * (1 + 1e-5), (g7, g9)
    tau = 512.0 / np.sqrt(g7 * g9)
    return k, c, -1j * tau


def test_need_host_at_later_check_and_alias(eng):
    k, c, dt = _later_host_problem()
    ex = k.expm(dt, c)
    priv = E.Engine(eng.device)        # a fresh context: no run-ahead hint (those are kept per context)
    try:
        h = E.mpse_heff()
        C.memmove(C.byref(h), C.byref(_hop(k).heff), C.sizeof(E.mpse_heff))
        keep = [priv.asdevice(k.l), priv.asdevice(k.r), priv.asdevice(k.cmo[0])]
        h.L, h.R, h.W0 = keep[0].ptr, keep[1].ptr, keep[2].ptr
        op = type("Op", (), {"heff": h})
        st, out, nv, d = _solve(priv, op, priv.asdevice(c), dt, 1e-10)
        assert st == 0 and d.get("host_later") == 1 and d.get("sync") == 1 and "host_first" not in d, d
        assert d.get("host_waits") == 2 and "alias_restart" not in d, d
        assert np.linalg.norm(out - ex) <= 1e-9 * np.linalg.norm(ex)
        # the same solve with out == C: an estimate went to out before the hand-over; C is put back first (a failed
        # asynchronous solve leaves no hint: the host waits at j = 6 again)
        ca = priv.asdevice(c)
        st2, out2, nv2, d2 = _solve(priv, op, ca, dt, 1e-10, out=ca)
        assert st2 == 0 and nv2 == nv and d2.get("host_later") == 1 and d2.get("alias_restart") == 1, d2
        assert np.array_equal(out2, out)
        del keep, ca
    finally:
        priv.close()


LONG_DIMS, LONG_TAU = (10, 12, 17), 5.0       # n = 2040, ~83 Krylov vectors at rtol = 1e-10, atol = 1e-12
LONG_TOL = (1e-10, 1e-12)


@pytest.fixture(scope="module")
def long_problem(eng):
    k = kron_problem(300, LONG_DIMS, True)
    c = _rand(np.random.default_rng(1), (k.n,), True)
    return k, _hop(k), c, k.expm(-1j * LONG_TAU, c)


def test_vector_limit_handover(eng, long_problem):
    k, hop, c, ex = long_problem
    st, out, nv, d = _solve(eng, hop, eng.asdevice(c), -1j * LONG_TAU, *LONG_TOL)
    assert st == 0 and 64 < nv <= 128, (st, nv)
    assert d.get("limit") == 1 and d.get("sync") == 1 and d.get("converged") == 1, d
    assert d.get("basis_growths", 0) >= 2, d
    assert _relerr(out, ex) < 1e-9
    ca = eng.asdevice(c)
    st2, out2, nv2, d2 = _solve(eng, hop, ca, -1j * LONG_TAU, *LONG_TOL, out=ca)
    assert st2 == 0 and nv2 == nv and d2.get("alias_restart") == 1 and d2.get("limit") == 1, d2
    assert np.array_equal(out2, out)


@pytest.mark.parametrize("max_dim", [8, 20, 63, 64, 65, 100])
def test_max_dim_on_async_centre(eng, long_problem, max_dim):
    k, hop, c, ex = long_problem
    st, out, nv, d = _solve(eng, hop, eng.asdevice(c), -1j * LONG_TAU, *LONG_TOL, max_dim=max_dim)
    if max_dim < 80:
        assert st == E.MPSE_ERR_NOCONV and nv == max_dim, (st, nv)
        assert d.get("noconv") == 1 and d.get("limit") == 1 and d.get("sync") == 1, d
        assert np.all(np.isfinite(out))
    else:
        assert st == 0 and nv <= max_dim and d.get("converged") == 1, (st, nv, d)
        assert _relerr(out, ex) < 1e-9
    # the same on a synchronous-size centre: NOCONV exactly at max_dim
    if max_dim <= 20:
        ks = kron_problem(301, SYNC_DIMS, True)
        cs = _rand(np.random.default_rng(2), (ks.n,), True)
        st, out, nv, d = _solve(eng, _hop(ks), eng.asdevice(cs), -8j, 1e-12, max_dim=max_dim)
        assert st == E.MPSE_ERR_NOCONV and nv == max_dim and d.get("noconv") == 1 and "limit" not in d, (st, nv, d)


def test_full_space(eng):
    """a bond of 2 x 3: the Krylov space reaches the whole space (j == n - 1) before any check can stop it"""
    k = kron_problem(120, (2, 3), True)
    c = _rand(np.random.default_rng(14), (k.n,), True)
    st, out, nv, d = _solve(eng, _hop(k), eng.asdevice(c), -0.7j, 1e-14)
    assert st == 0 and nv == 6 and d.get("full_space") == 1 and d.get("sync") == 1, (st, nv, d)
    assert _relerr(out, k.expm(-0.7j, c)) <= 20 * EPS * 7


# =============================================================================================== 4. matvec paths

# (name, centre dims, complex, what shows that the path ran)
MATVECS = [
    ("small_one_launch", (8, 5, 9), True, None),
    ("contraction_plans", (40, 7, 130), True, "gemm"),           # n = 36 400 > 32 768: the plans' products
    ("two_site", (6, 3, 4, 7), True, None),
    ("bond", (20, 24), True, None),
    ("fused_bond", (192, 192), True, "fused_bond"),              # k_heff0_fused, result in tile-masked parts
    ("fused_two_level", (128, 2, 192), True, "fused_site"),      # d = 2 one-site centre with the site hint
    ("folded_d16", (256, 16, 256), True, "grouped"),             # d = 16 site with the hint: the folded plan
    ("real_odd", (7, 5, 9), False, "unvec"),
    ("real_even", (8, 5, 9), False, None),
]


@pytest.mark.parametrize("name,dims,cplx,shows", MATVECS, ids=[m[0] for m in MATVECS])
def test_matvec_paths(eng, name, dims, cplx, shows):
    k = kron_problem(60, dims, cplx)
    hop = _hop(k)               # (one-site Kron sites are host arrays: Hop describes them with mpse_mpo_site_hint)
    rng = np.random.default_rng(9)
    kk = 3
    c, lam, coef, U = _eig_start(k, kk, rng, cplx)
    al, be = _lanczos(k.apply, c, 10)
    tau = 0.7 / _gersh(al, be)
    dt = -1j * tau if cplx else tau
    f0, gp0 = eng.heff_fused_stats(), eng.gemm_path_stats()
    st, out, nv, d = _solve(eng, hop, eng.asdevice(c), dt, 1e-14)
    assert st == 0 and nv == kk, (st, nv, d)
    assert _relerr(out, _exact_eig(dt, lam, coef, U)) <= 20 * EPS * (kk + 1)
    assert d.get("async_done") == 1 and d.get("breakdown_async") == 1, d
    g = _rand(rng, (k.n,), cplx)
    width = sum(float(e.max() - e.min()) for e in k.ev)
    gdt = (-3j if cplx else -3.0) / width
    st, out, nv, d2 = _solve(eng, hop, eng.asdevice(g), gdt, 1e-10)
    ex = k.expm(gdt, g)
    assert st == 0 and np.linalg.norm(out - ex) <= 1e-9 * np.linalg.norm(ex) + 1e-13 * np.linalg.norm(g)
    assert d2.get("async_done") == 1, d2
    f1, gp1 = eng.heff_fused_stats(), eng.gemm_path_stats()
    if shows == "unvec":
        assert d.get("update_unvec", 0) > 0 and d2.get("update_unvec", 0) > 0, (d, d2)
    else:
        assert "update_unvec" not in d and "update_unvec" not in d2, (d, d2)
    if shows == "gemm":
        assert gp1["launches"] > gp0["launches"]
    if shows == "grouped":
        assert gp1["grouped"] > gp0["grouped"], (gp0, gp1)
    if shows in ("fused_bond", "fused_site"):
        i = 0 if shows == "fused_bond" else 1
        assert f1[i] - f0[i] >= nv + kk, (f0, f1)
        assert d.get("update_parts", 0) >= kk and d2.get("update_parts", 0) >= nv, (d, d2)   # (tile-masked parts)
    else:
        assert f1 == f0, (f0, f1)
        if shows != "grouped":           # (the folded plan may deliver its result in two halves)
            assert "update_parts" not in d and "update_parts" not in d2, (d, d2)


def test_centre_mask_vmask(eng):
    """a centre mask (mpse_expm_centre_mask) on a centre whose factors are block-diagonal by charge, so that H keeps
    the sector: the update kernel applies the mask to the vectors (counter), the result matches the exponential and is
    exactly zero in every tile the mask leaves out"""
    Dl, d, Dr = 32, 4, 64
    chl, chs, chr_ = np.arange(Dl) // 16, np.arange(d), np.arange(Dr) // 32
    k = kron_problem(130, (Dl, d, Dr), True, charges=[chl, chs, chr_])
    allowed = ((chl[:, None, None] + chs[None, :, None] + chr_[None, None, :]) == 1).reshape(Dl, d * Dr)
    hop = _hop(k)
    hop.cmask = centre_tile_mask(eng, (chl[:, None] + chs[None, :]).reshape(-1, 1), chr_[:, None], np.array([1]),
                                 k.shape)
    assert hop.cmask is not None
    tiles = np.zeros(((Dl + 15) // 16, (d * Dr + 63) // 64), dtype=bool)
    for a, col in zip(*np.nonzero(allowed)):
        tiles[a // 16, col // 64] = True
    assert not tiles.all()                                  # the mask leaves tiles out
    outside_tiles = ~np.repeat(np.repeat(tiles, 16, 0), 64, 1)[:Dl, :d * Dr]
    c = _rand(np.random.default_rng(15), (Dl, d * Dr), True) * allowed
    for dt in (-0.3j, 0.2 - 0.1j):
        st, out, nv, dd = _solve(eng, hop, eng.asdevice(c.reshape(k.shape)), dt, 1e-10)
        assert st == 0 and dd.get("update_vmask", 0) > 0 and dd.get("async_done") == 1, (st, dd)
        ex = k.expm(dt, c.ravel())
        assert np.linalg.norm(out - ex) <= 1e-9 * np.linalg.norm(ex)
        o = out.reshape(Dl, d * Dr)
        assert np.all(o[outside_tiles] == 0)
        assert np.abs(o[~allowed]).max() <= 1e-12 * np.abs(o).max()


def test_centre_mask_lifetime(eng):
    """a centre mask serves exactly the one mpse_expm_lanczos that follows it (the problem of test_centre_mask_vmask):
    the second solve after it runs without; a batch between the mask and its solve neither uses nor drops it; a solve
    that is refused on its arguments uses it up"""
    Dl, d, Dr = 32, 4, 64
    chl, chs, chr_ = np.arange(Dl) // 16, np.arange(d), np.arange(Dr) // 32
    k = kron_problem(130, (Dl, d, Dr), True, charges=[chl, chs, chr_])
    allowed = ((chl[:, None, None] + chs[None, :, None] + chr_[None, None, :]) == 1).reshape(Dl, d * Dr)
    hop = _hop(k)                                           # (no cmask attribute: _solve sets no mask by itself)
    cmask = centre_tile_mask(eng, (chl[:, None] + chs[None, :]).reshape(-1, 1), chr_[:, None], np.array([1]), k.shape)
    assert cmask is not None
    c = _rand(np.random.default_rng(15), (Dl, d * Dr), True) * allowed
    dt = -0.3j
    ex = k.expm(dt, c.ravel())

    def set_mask():
        eng._check(eng.lib.mpse_expm_centre_mask(eng.ctx, cmask.ptr, cmask.nbytes))

    def solve(masked):
        st, out, nv, dd = _solve(eng, hop, eng.asdevice(c.reshape(k.shape)), dt, 1e-10)
        assert st == 0 and dd.get("async_done") == 1, (st, dd)
        assert (dd.get("update_vmask", 0) > 0) == masked, dd
        assert np.linalg.norm(out - ex) <= 1e-9 * np.linalg.norm(ex)

    # consumed once
    set_mask()
    solve(True)
    solve(False)
    # survives a batch, whose members do not use it
    set_mask()
    devs = [eng.asdevice(c.reshape(k.shape)) for _ in range(2)]
    st, outs, nvs, dd, (nb, ns) = _batch(eng, [hop, hop], devs, dt, 1e-10)
    assert st == 0 and nb + ns == 2 and "update_vmask" not in dd, (st, nb, ns, dd)
    for o in outs:
        assert np.linalg.norm(o - ex) <= 1e-9 * np.linalg.norm(ex)
    solve(True)
    solve(False)
    # cleared by a solve that is refused before any launch: out overlaps C without being C
    set_mask()
    buf = eng.asdevice(np.concatenate([c.ravel(), np.zeros(k.n)]))
    nvc = C.c_int()
    s0, g0 = eng.lanczos_path_stats(), eng.gemm_path_stats()
    st = eng.lib.mpse_expm_lanczos(eng.ctx, buf.code, C.byref(hop.heff), dt.real, dt.imag, buf.ptr, buf.ptr + 16 * 64,
                                   1e-10, 0.0, 0, C.byref(nvc))
    assert st == E.MPSE_ERR_ARG
    assert eng.lanczos_path_stats() == s0 and eng.gemm_path_stats() == g0
    assert np.array_equal(buf.to_host()[:k.n], c.ravel())
    solve(False)


# =============================================================================================== 5. run-ahead hint

def test_run_ahead_hint_changes_waits_only(eng):
    """the same solve after predecessors of the same class (nsite, n, dtype) with shorter, equal and longer Krylov
    dimensions: bitwise the same result; the host waits differ"""
    k = kron_problem(70, (8, 5, 10), True)
    hop = _hop(k)
    rng = np.random.default_rng(6)
    c = eng.asdevice(_rand(rng, (k.n,), True))
    p = eng.asdevice(_rand(rng, (k.n,), True))
    res, waits = [], []
    for pre_dt in (-0.05j, -0.6j, -3.0j):
        st, _, npre, _ = _solve(eng, hop, p, pre_dt, 1e-10)
        assert st == 0
        st, out, nv, d = _solve(eng, hop, c, -0.6j, 1e-10)
        assert st == 0 and d.get("async_done") == 1
        res.append(out)
        waits.append(d.get("host_waits"))
    assert all(np.array_equal(res[0], r) for r in res[1:])
    assert len(set(waits)) > 1, waits
    assert _relerr(res[0], k.expm(-0.6j, c.to_host())) < 1e-9


# =============================================================================================== 6. batched

def test_batched_members_across_bands(eng):
    """members of one shape: bands (0, 1/2], s = 1, 3, 6, 8 and the host (E0 shifts, one dt), a breakdown member;
    each bitwise its single solve, within the exact bounds; out == C gives the same"""
    cplx = True
    k0 = kron_problem(80, ASYNC_DIMS, cplx)
    rng = np.random.default_rng(8)
    g = _rand(rng, (k0.n,), cplx)
    al, be = _lanczos(k0.apply, g, 30)
    g0 = _gersh(al, be)
    tau = 0.35 / g0
    dt = -1j * tau
    ks, cs = [], []
    for target in (0.0, 2.8, 11.3, 90.5, 362.0, 600.0):
        e0 = 0.0 if target == 0.0 else target / tau - g0
        ks.append(kron_problem(80, ASYNC_DIMS, cplx, shift=e0))
        cs.append(_rand(rng, (k0.n,), cplx))
    kb = kron_problem(81, ASYNC_DIMS, cplx)
    exact_members = []       # breakdown members: 2, 5 and 8 exact eigenvectors (before, at and after the merged check)
    for kk in (2, 5, 8):
        cb, lam, coef, U = _eig_start(kb, kk, rng, cplx)
        exact_members.append((len(ks), kk, lam, coef, U))
        ks.append(kb)
        cs.append(cb)
    hops = [_hop(k) for k in ks]
    devs = [eng.asdevice(c) for c in cs]
    singles = [_solve(eng, h, c, dt, 1e-10) for h, c in zip(hops, devs)]
    st, outs, nvs, d, (nb, ns) = _batch(eng, hops, devs, dt, 1e-10)
    assert st == 0 and nb + ns == len(hops) and nb >= 2, (st, nb, ns)
    assert ns >= 1 and d.get("sync", 0) >= 1, d      # the host member: the synchronous solve, from the batch
    for i, (s1, o, nv) in enumerate(zip(singles, outs, nvs)):
        assert s1[0] == 0 and np.array_equal(s1[1], o) and s1[2] == nv, i
        ex = ks[i].expm(dt, cs[i])
        assert _nrm(o - ex) <= 10 * 1e-10 * _nrm(ex) + 1e-13 * _nrm(cs[i]), i
    for i, kk, lam, coef, U in exact_members:
        assert nvs[i] == kk and _relerr(outs[i], _exact_eig(dt, lam, coef, U)) <= 20 * EPS * (kk + 1), (i, kk)
    # out == C
    devs2 = [eng.asdevice(c) for c in cs]
    st, outs2, nvs2, _, _ = _batch(eng, hops, devs2, dt, 1e-10, outs=devs2)
    assert st == 0 and nvs2 == nvs
    assert all(np.array_equal(a, b) for a, b in zip(outs, outs2))


def test_batch_grows_and_member_leaves_at_limit(eng, long_problem):
    """three members of LONG_DIMS under one dt whose single solves need 17 .. 32, 33 .. 63 and more than 64 vectors:
    the slab of the batch grows (it starts at 16 vectors: a short solve of the class sets the run-ahead hint first),
    two members finish at different checks and the third leaves at the 64-vector limit for the synchronous solve.
    The members differ by an energy shift.  A shift alone cannot move the Krylov dimension under a real-time step
    (exp(dt (H + E)) = exp(dt E) exp(dt H): the same Krylov space, estimates that differ by a phase), so the first two
    also have their level spacings scaled by 0.12 and 0.4 (|dt| x spectral width 12 and 41 instead of 103; a host
    Lanczos with the engine's checks gives 27 and 47 vectors); the third is the problem of test_vector_limit_handover."""
    k3, hop3, c3, ex3 = long_problem
    dt = -1j * LONG_TAU
    base = [0.71, 0.43, 0.59, 0.37]
    rng = np.random.default_rng(12)
    ks = [kron_problem(300, LONG_DIMS, True, shift=7.0, spacing=[0.12 * s for s in base]),
          kron_problem(300, LONG_DIMS, True, shift=3.0, spacing=[0.4 * s for s in base]), k3]
    cs = [_rand(rng, (k3.n,), True), _rand(rng, (k3.n,), True), c3]
    exs = [ks[0].expm(dt, cs[0]), ks[1].expm(dt, cs[1]), ex3]
    hops = [_hop(ks[0]), _hop(ks[1]), hop3]
    devs = [eng.asdevice(c) for c in cs]
    singles = [_solve(eng, h, c, dt, *LONG_TOL) for h, c in zip(hops, devs)]
    assert all(s[0] == 0 for s in singles)
    assert 16 < singles[0][2] <= 32 and 32 < singles[1][2] < 64 and 64 < singles[2][2] <= 128, [s[2] for s in singles]
    assert singles[2][3].get("limit") == 1 and singles[2][3].get("sync") == 1, singles[2][3]
    cshort, _, _, _ = _eig_start(k3, 3, rng, True)

    def short_solve():           # leaves the hint of the class at 3: the next solve starts with room for 16 vectors
        st, _, nv, _ = _solve(eng, hop3, eng.asdevice(cshort), dt, 1e-14)
        assert st == 0 and nv <= 8, (st, nv)

    short_solve()
    st, outs, nvs, d, (nb, ns) = _batch(eng, hops, devs, dt, *LONG_TOL)
    assert st == 0 and nb == 2 and ns == 1, (st, nb, ns)
    # the third member: the synchronous solve, straight from the batch (whose own loop counts no paths)
    assert d.get("sync") == 1 and "limit" not in d and d.get("converged") == 1, d
    for i, (s1, o, nv) in enumerate(zip(singles, outs, nvs)):
        assert np.array_equal(s1[1], o) and s1[2] == nv, i
        assert _relerr(o, exs[i]) < 1e-9, i
    # out == C
    short_solve()
    devs2 = [eng.asdevice(c) for c in cs]
    st, outs2, nvs2, _, (nb2, ns2) = _batch(eng, hops, devs2, dt, *LONG_TOL, outs=devs2)
    assert st == 0 and nvs2 == nvs and (nb2, ns2) == (2, 1)
    assert all(np.array_equal(a, b) for a, b in zip(outs, outs2))


# =============================================================================================== 7. edges

@pytest.mark.parametrize("path", ["sync", "async"])
def test_alias_and_partial_overlap(eng, path):
    k = kron_problem(90, SYNC_DIMS if path == "sync" else ASYNC_DIMS, True)
    hop = _hop(k)
    c = _rand(np.random.default_rng(10), (k.n,), True)
    st, out, nv, d = _solve(eng, hop, eng.asdevice(c), -0.4j, 1e-10)
    ca = eng.asdevice(c)
    st2, out2, nv2, d2 = _solve(eng, hop, ca, -0.4j, 1e-10, out=ca)
    assert st == st2 == 0 and nv == nv2 and np.array_equal(out, out2)
    assert _relerr(out, k.expm(-0.4j, c)) < 1e-9
    # an out that overlaps C one element further on is refused, and C is left alone
    buf = eng.asdevice(np.concatenate([c, np.zeros(1)]))
    nvc = C.c_int()
    st3 = eng.lib.mpse_expm_lanczos(eng.ctx, buf.code, C.byref(hop.heff), 0.0, -0.4, buf.ptr, buf.ptr + 16, 1e-10, 0.0,
                                    0, C.byref(nvc))
    assert st3 == E.MPSE_ERR_ARG
    assert np.array_equal(buf.to_host()[:k.n], c)


@pytest.mark.parametrize("cplx", [True, False], ids=["c128", "f64"])
@pytest.mark.parametrize("path", ["sync", "async"])
def test_power_of_two_scaling(eng, path, cplx):
    """C scaled by 2^j with atol = 0: bitwise 2^j times the unscaled result while |C|^2 is a normal double below 1e300
    and the elements stay normal; beyond that range the start vector is rescaled (counter) and the result is still
    bitwise 2^j times, as long as its elements are normal"""
    k = kron_problem(100, SYNC_DIMS if path == "sync" else ASYNC_DIMS, cplx)
    hop = _hop(k)
    c = _rand(np.random.default_rng(12), (k.n,), cplx)
    dt = (0.3 - 0.9j) if cplx else -0.3

    def scaled(x, j):
        return np.ldexp(x.real, j) + 1j * np.ldexp(x.imag, j) if cplx else np.ldexp(x, j)

    st, base, nv, _ = _solve(eng, hop, eng.asdevice(c), dt, 1e-10)
    assert st == 0
    assert _relerr(base, k.expm(dt, c)) < 1e-9
    n2 = float(np.vdot(c, c).real)
    parts = [c.real, c.imag, base.real, base.imag] if cplx else [c, base]
    lo = min(float(np.abs(x).min()) for x in parts)
    hi = max(np.abs(c).max(), np.abs(base).max())
    for j in (-1000, -540, -520, -480, -200, -37, 1, 5, 100, 300, 480, 500, 520, 1000):
        cj = scaled(c, j)
        st, out, nvj, d = _solve(eng, hop, eng.asdevice(cj), dt, 1e-10)
        in_range = -1022 <= math.log2(n2) + 2 * j < math.log2(1e300)
        normal = math.log2(lo) + j >= -1022 and math.log2(hi) + j < 1000
        if st != 0:
            assert not in_range and st == E.MPSE_ERR_ARG, (j, st)
            continue
        assert np.all(np.isfinite(out)), j
        want = scaled(base, j)
        if normal:
            assert np.array_equal(out, want) and nvj == nv, (j, d)
        else:
            assert _nrm(out - want) <= 1e-12 * _nrm(want), j
        assert ("rescaled" in d) == (not in_range), (j, d)


@pytest.mark.parametrize("path", ["sync", "async"])
@pytest.mark.parametrize("bad", ["zero", "nan", "inf"])
def test_bad_start_vectors(eng, path, bad):
    """zero, NaN and inf start vectors are errors on both paths, in both types; the path that met them is counted
    and no solve on a rescaled vector starts"""
    for cplx in (True, False):
        k = kron_problem(110, SYNC_DIMS if path == "sync" else ASYNC_DIMS, cplx)
        c = _rand(np.random.default_rng(13), (k.n,), cplx)
        if bad == "zero":
            c[:] = 0
        else:
            c[7] = np.nan if bad == "nan" else np.inf
        st, out, nv, d = _solve(eng, _hop(k), eng.asdevice(c), -0.3j if cplx else -0.3, 1e-10)
        assert st == E.MPSE_ERR_ARG, (cplx, st, d)
        assert "rescaled" not in d and "async_done" not in d and "converged" not in d, d
        if path == "sync":
            assert d.get("sync") == 1, d
        else:
            assert "sync" not in d and d.get("host_waits", 0) >= 1, d
