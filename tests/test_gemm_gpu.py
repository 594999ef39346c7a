"""Every launch path of the contraction kernel (mpse_gemm.hip: gemm_impl) against exact references.

Each row of CASES names the paths its launch must take; the test asserts the deltas of ``mpse_gemm_path_stats`` so
the table cannot drift silently when a threshold or the number of compute units changes.  Every case runs in the four
operand type pairs and is checked three ways:
  * exact: integer operands (|x| <= 8 in both parts), integer or power-of-two alpha / beta, integer C0 - every partial
    sum is an integer below 2**53, so any path (split-K included) must reproduce the int64 product bit for bit;
  * rounding: standard-normal operands against float64 NumPy, element by element inside
    c * gamma(K + 2) * (|alpha| |A| @ |B| + |beta| |C0|) (c = 2 real, 4 complex: the kernel's 3M scheme);
  * work: the K tiles the kernel multiplied (``prof_get``) equal the dense count, or with a skip hint the count of K
    tiles occupied on the scanned sides (next_kt: a K tile is visited when both scanned 64 x 16 operand tiles hold a
    non-zero).
Operands live in flat buffers whose unused elements are NaN (a misaddressed read poisons the result); the unused
elements of C hold a sentinel that must survive the call.
"""
import ctypes as C

import numpy as np
import pytest

from renormalizer_amd import engine as E

from gemm_policy import CASES, _shape_preconditions, expected_paths   # (tests/gemm_policy.py)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DTYPES = [(False, False), (True, False), (False, True), (True, True)]
DT_IDS = ["f64xf64", "c128xf64", "f64xc128", "c128xc128"]
C_FILL = 777.25


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def gamma(n):
    return n * U / (1 - n * U)


def one(ext, s):
    return (ext, max(ext, 1), 0, s)


def two(ext, lo, s_hi, s_lo):
    return (ext, lo, s_hi, s_lo)


def _offsets(m):
    ext, lo, s_hi, s_lo = m
    i = np.arange(ext, dtype=np.int64)
    return (i // max(lo, 1)) * s_hi + (i % max(lo, 1)) * s_lo


class Placed:
    """Logical (batch, R, S) values at base + b * sb + off_r[r] + off_s[s] of a flat device buffer whose other
    elements hold `fill`."""

    def __init__(self, eng, vals, rmap, smap, sb, fill):
        self.eng, self.dtype = eng, vals.dtype
        nb = vals.shape[0]
        rel = (np.arange(nb, dtype=np.int64)[:, None, None] * sb + _offsets(rmap)[None, :, None]
               + _offsets(smap)[None, None, :])
        base = -int(rel.min()) if rel.size and rel.min() < 0 else 0
        self.pos = rel + base
        assert np.unique(self.pos).size == self.pos.size, "operand elements alias"
        self.flat = np.full(int(self.pos.max()) + 1 if self.pos.size else 1, fill, dtype=vals.dtype)
        self.flat[self.pos] = vals
        self.dev = eng.asdevice(self.flat)
        self.ptr = self.dev.ptr + base * vals.dtype.itemsize

    def read(self):
        """(logical values, unused elements unchanged bitwise)"""
        f = self.dev.to_host()
        gap = np.ones(f.size, dtype=bool)
        gap[self.pos.ravel()] = False
        same = np.array_equal(f[gap].view(np.int64), self.flat[gap].view(np.int64))
        return f[self.pos], same


def _gemm(eng, ca, cb, conj, maps, batch, sbs, alpha, beta, hint, pa, pb, pc, dtype_a=None):
    d = E.mpse_gemm_desc()
    d.dtype_a = (E.C128 if ca else E.F64) if dtype_a is None else dtype_a
    d.dtype_b = E.C128 if cb else E.F64
    d.conj_a, d.conj_b = int(conj[0]), int(conj[1])
    d.m_a, d.k_a, d.k_b, d.n_b, d.m_c, d.n_c = (E.mpse_index(*m) for m in maps)
    d.batch, (d.sb_a, d.sb_b, d.sb_c) = batch, sbs
    alpha, beta = complex(alpha), complex(beta)
    d.alpha_re, d.alpha_im, d.beta_re, d.beta_im = alpha.real, alpha.imag, beta.real, beta.imag
    d.skip_zero_tiles = hint
    return eng.lib.mpse_gemm(eng.ctx, C.byref(d), pa, pb, pc)


def _ktiles(eng):
    p = eng.prof_get()
    return sum(p[n]["ktiles"] for n in ("f64xf64", "c128xf64", "f64xc128", "c128xc128"))


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


# ------------------------------------------------------------------------------------------------ operand layouts
def layout(kind, M, N, K, batch):
    """index maps (m_a, k_a, k_b, n_b, m_c, n_c) and batch strides of the named storage"""
    if kind == "rowmajor":
        return (one(M, K), one(K, 1), one(K, N), one(N, 1), one(M, N), one(N, 1)), (M * K, K * N, M * N)
    if kind == "gaps":        # padded rows and batch strides with gaps
        return ((one(M, K + 3), one(K, 1), one(K, N + 2), one(N, 1), one(M, N + 1), one(N, 1)),
                (M * (K + 3) + 5, K * (N + 2) + 7, M * (N + 1) + 3))
    if kind == "trans":       # A stored (K, M), B stored (N, K): rows of A / columns of B contiguous
        return (one(M, 1), one(K, M), one(K, 1), one(N, K), one(M, N), one(N, 1)), (M * K, K * N, M * N)
    if kind == "twolevel":    # A (Mh, Kh, 5, 13), B (Kh, Nh, 13, 7), C (Mh, Nh, 5, 7)
        Kh, Nh = K // 13, N // 7
        assert M % 5 == 0 and K % 13 == 0 and N % 7 == 0 and Kh > 1 and Nh > 1
        return ((two(M, 5, Kh * 65, 13), two(K, 13, 65, 1), two(K, 13, Nh * 91, 7), two(N, 7, 91, 1),
                 two(M, 5, Nh * 35, 7), two(N, 7, 35, 1)), (M * K, K * N, M * N))
    if kind == "reversed":    # A and B read backwards from their last element
        return (one(M, -K), one(K, -1), one(K, -N), one(N, -1), one(M, N), one(N, 1)), (-M * K, -K * N, M * N)
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------ data
def _blocks(rng, rows, cols, nr, nc):
    """0/1 block pattern (quantum-number-like sectors at ragged boundaries), about half the blocks filled"""
    rb = np.unique(np.r_[0, np.sort(rng.choice(np.arange(1, rows), nr - 1, replace=False)), rows])
    cb = np.unique(np.r_[0, np.sort(rng.choice(np.arange(1, cols), nc - 1, replace=False)), cols])
    m = np.zeros((rows, cols), dtype=bool)
    for i in range(len(rb) - 1):
        for j in range(len(cb) - 1):
            if rng.random() < 0.5:
                m[rb[i]:rb[i + 1], cb[j]:cb[j + 1]] = True
    return m


def _ints(rng, shape, cplx):
    a = rng.integers(-8, 9, shape)
    return (a, rng.integers(-8, 9, shape)) if cplx else (a, np.zeros(shape, dtype=np.int64))


def _normal(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def _compose(re, im, cplx):
    """float64 / complex128 array with exactly these parts"""
    if not cplx:
        return np.asarray(re, dtype=np.float64)
    out = np.empty(np.shape(re), np.complex128)
    out.real, out.imag = re, im
    return out


def _as_float(re, im, cplx):
    return _compose(re.astype(np.float64), im.astype(np.float64), cplx)


def _real_of(z):
    """a non-zero real stand-in for a complex scalar (real results use alpha_re / beta_re only)"""
    z = complex(z)
    return z.real if z.real != 0 else z.imag


def _int_product(a, b, conj):
    """exact opA(A) @ opB(B) in int64: a, b = (re, im) pairs"""
    ar, ai = a
    br, bi = b
    ai = -ai if conj[0] else ai
    bi = -bi if conj[1] else bi
    return np.matmul(ar, br) - np.matmul(ai, bi), np.matmul(ar, bi) + np.matmul(ai, br)


def _occupied(nz, rows_axis_len, K):
    """(batch, tiles, K tiles) occupancy of (batch, rows, K) non-zero flags"""
    nb = nz.shape[0]
    t, nkt = -(-rows_axis_len // 64), -(-K // 16)
    p = np.zeros((nb, t * 64, nkt * 16), dtype=bool)
    p[:, :rows_axis_len, :K] = nz
    return p.reshape(nb, t, 64, nkt, 16).any(axis=(2, 4))


def expected_ktiles(M, N, K, batch, hint, a_nz, b_nz):
    nkt = -(-K // 16)
    tm, tn = -(-M // 64), -(-N // 64)
    if not hint:
        return batch * tm * tn * nkt
    oa = _occupied(a_nz, M, K) if hint & 1 else np.ones((batch, tm, nkt), dtype=bool)
    ob = _occupied(np.swapaxes(b_nz, 1, 2), N, K) if hint & 2 else np.ones((batch, tn, nkt), dtype=bool)
    return int(np.einsum("btk,bsk->", oa.astype(np.int64), ob.astype(np.int64)))


class SpanB:
    """B(k, j) at k * s + j in one device allocation with 2 s * element size >= 4.3 GB; only the K rows are written"""

    def __init__(self, eng, vals, cplx):
        K, N = vals.shape[1:]
        esz = 16 if cplx else 8
        self.s = -(-int(4.3e9) // (2 * esz))
        self.dev = eng.empty(((K - 1) * self.s + N,), np.complex128 if cplx else np.float64)
        for k in range(K):
            row = np.ascontiguousarray(vals[0, k])
            eng._check(eng.lib.mpse_memcpy_h2d(eng.ctx, self.dev.ptr + k * self.s * esz, row.ctypes.data, row.nbytes))
        self.ptr = self.dev.ptr


def _run_case(eng, name, ca, cb, rng):
    n_cu = eng.n_cu
    dims, kind, sparse, hints, alpha, beta = CASES[name]
    M, N, K, batch = dims(n_cu)
    _shape_preconditions(name, n_cu, M, N, K, batch)
    cc = ca or cb
    if not cc:
        alpha, beta = _real_of(alpha), _real_of(beta)
    span = kind == "span"
    maps, sbs = layout("rowmajor" if span else kind, M, N, K, batch)     # (span: B's K stride set by SpanB)
    ma = _blocks(rng, M, K, 7, 5) if sparse else np.ones((M, K), dtype=bool)
    mb = _blocks(rng, K, N, 5, 6) if sparse else np.ones((K, N), dtype=bool)
    shp_a, shp_b, shp_c = (batch, M, K), (batch, K, N), (batch, M, N)
    conj_exact = (ca, cb)
    conj_round = (False, cb)
    bound_c = 4.0 if cc else 2.0
    report = []

    def launch(a_vals, b_vals, c_vals, conj, hint):
        dA = Placed(eng, a_vals, maps[0], maps[1], sbs[0], np.nan)
        if span:
            dB = SpanB(eng, b_vals, cb)
            bmaps = (one(K, dB.s), maps[3])
        else:
            dB = Placed(eng, b_vals, maps[2], maps[3], sbs[1], np.nan)
            bmaps = maps[2:4]
        dC = Placed(eng, c_vals, maps[4], maps[5], sbs[2], C_FILL)
        st0 = eng.gemm_path_stats()
        kt0 = _ktiles(eng)
        st = _gemm(eng, ca, cb, conj, (maps[0], maps[1]) + bmaps + maps[4:], batch, sbs, alpha, beta, hint,
                   dA.ptr, dB.ptr, dC.ptr)
        assert st == 0, eng.lib.mpse_last_error(eng.ctx)
        kt = _ktiles(eng) - kt0
        paths = _delta(st0, eng.gemm_path_stats())
        out, gaps_ok = dC.read()
        assert gaps_ok, f"{name}: elements of C outside the result changed"
        del dB
        if span:
            eng.free_all_blocks()
        return out, paths, kt

    round_ref = None
    eng.prof_enable(1)
    try:
        for hint in hints:
            want = expected_paths(name, n_cu, M, N, K, batch, hint)
            # exact
            a = _ints(rng, shp_a, ca)
            b = _ints(rng, shp_b, cb)
            a = (a[0] * ma, a[1] * ma)
            b = (b[0] * mb, b[1] * mb)
            c0 = _ints(rng, shp_c, cc)
            xr, xi = _int_product(a, b, conj_exact)
            assert max(np.abs(xr).max(), np.abs(xi).max()) < 2 ** 40
            x = _as_float(xr, xi, cc)
            ref = alpha * x + beta * _as_float(*c0, cc)
            a_f, b_f, c_f = _as_float(*a, ca), _as_float(*b, cb), _as_float(*c0, cc)
            out, paths, kt = launch(a_f, b_f, c_f, conj_exact, hint)
            report.append(f"{name} hint {hint}: {paths} ktiles {kt}")
            assert paths == want, f"{name} hint {hint}: path counters {paths}, expected {want}"
            a_nz = (a[0] != 0) | (a[1] != 0)
            b_nz = (b[0] != 0) | (b[1] != 0)
            assert kt == expected_ktiles(M, N, K, batch, hint, a_nz, b_nz), (name, hint, kt)
            bad = np.argwhere(out != ref)
            assert bad.size == 0, f"{name} hint {hint}: {len(bad)} inexact elements, first {bad[:3].tolist()}"
            out2, paths2, _ = launch(a_f, b_f, c_f, conj_exact, hint)
            assert paths2 == want and np.array_equal(out2.view(np.int64), out.view(np.int64)), "repeated call differs"
            # rounding
            if round_ref is None:
                ar = _normal(rng, shp_a, ca) * ma
                br = _normal(rng, shp_b, cb) * mb
                cr = _normal(rng, shp_c, cc)
                opb = br.conj() if conj_round[1] else br
                exact = alpha * np.matmul(ar, opb) + beta * cr
                bound = bound_c * gamma(K + 2) * (abs(alpha) * np.matmul(np.abs(ar), np.abs(br)) + abs(beta) * np.abs(cr))
                round_ref = (ar, br, cr, exact, bound)
            ar, br, cr, exact, bound = round_ref         # the same operands for every hint: bitwise invariance
            out, paths, _ = launch(ar, br, cr, conj_round, hint)
            assert paths == want
            err = np.abs(out - exact)
            assert np.all(err <= bound), f"{name} hint {hint}: error {float((err / bound).max()):.3g} x the bound"
            if hint == hints[0]:
                first = out
            else:
                assert np.array_equal(out, first), f"{name}: skip hint {hint} differs from hint {hints[0]}"
    finally:
        eng.prof_enable(0)
    print("\n".join(report))
    return report


@pytest.mark.parametrize("ca,cb", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_gemm_path(eng, name, ca, cb):
    _run_case(eng, name, ca, cb, np.random.default_rng(4 * list(CASES).index(name) + DTYPES.index((ca, cb))))


def test_every_path_counter_reached():
    """the table covers every counter except the grouped launches (those belong to the one-site matvec plans)"""
    reached = set()
    for name, (dims, kind, sparse, hints, *_rest) in CASES.items():
        M, N, K, batch = dims(256)
        for h in hints:
            reached |= set(expected_paths(name, 256, M, N, K, batch, h))
    assert reached == set(E.Engine.GEMM_PATHS) - {"grouped", "grouped_split2"}


# ------------------------------------------------------------------------------------------------ edges
def _simple(eng, ca, cb, M, N, K, a, b, c, alpha, beta, conj=(False, False), hint=0, batch=1):
    maps, sbs = layout("rowmajor", M, N, K, batch)
    dA = Placed(eng, a, maps[0], maps[1], sbs[0], np.nan)
    dB = Placed(eng, b, maps[2], maps[3], sbs[1], np.nan)
    dC = Placed(eng, c, maps[4], maps[5], sbs[2], C_FILL)
    st0 = eng.gemm_path_stats()
    st = _gemm(eng, ca, cb, conj, maps, batch, sbs, alpha, beta, hint, dA.ptr, dB.ptr, dC.ptr)
    assert st == 0, eng.lib.mpse_last_error(eng.ctx)
    out, gaps_ok = dC.read()
    assert gaps_ok
    return out, _delta(st0, eng.gemm_path_stats())


def _exact_inputs(rng, M, N, K, ca, cb, batch=1):
    a, b = _ints(rng, (batch, M, K), ca), _ints(rng, (batch, K, N), cb)
    c0 = _ints(rng, (batch, M, N), ca or cb)
    return a, b, c0


@pytest.mark.parametrize("ca,cb", DTYPES, ids=DT_IDS)
def test_k_zero_gives_beta_c(eng, ca, cb):
    """K = 0: the K loop is empty (kt_end = 0), no operand element is read, C = beta C0"""
    rng = np.random.default_rng(5)
    cc = ca or cb
    beta = (-2 + 1j) if cc else -2.0
    c0 = _as_float(*_ints(rng, (1, 70, 50), cc), cc)
    a = np.zeros((1, 70, 0), np.complex128 if ca else np.float64)
    b = np.zeros((1, 0, 50), np.complex128 if cb else np.float64)
    for bt in (beta, 0.0):
        out, paths = _simple(eng, ca, cb, 70, 50, 0, a, b, c0, 3.0, bt)
        assert paths.get("launches") == 1
        assert np.array_equal(out, bt * c0)


@pytest.mark.parametrize("ca,cb", DTYPES, ids=DT_IDS)
def test_empty_extents_leave_c_untouched(eng, ca, cb):
    """M = 0, N = 0 or batch = 0: nothing is launched and C keeps its values"""
    rng = np.random.default_rng(6)
    M, N, K = 40, 30, 20
    maps, sbs = layout("rowmajor", M, N, K, 1)
    dA = Placed(eng, _normal(rng, (1, M, K), ca), maps[0], maps[1], 0, np.nan)
    dB = Placed(eng, _normal(rng, (1, K, N), cb), maps[2], maps[3], 0, np.nan)
    c0 = _normal(rng, (1, M, N), ca or cb)
    dC = Placed(eng, c0, maps[4], maps[5], 0, C_FILL)
    no_m = (one(0, K), maps[1], maps[2], maps[3], one(0, N), maps[5])
    no_n = (maps[0], maps[1], one(K, 0), one(0, 1), maps[4], one(0, 1))
    for m, batch in ((no_m, 1), (no_n, 1), (maps, 0)):
        st0 = eng.gemm_path_stats()
        assert _gemm(eng, ca, cb, (0, 0), m, batch, sbs, 1.0, 1.0, 3, dA.ptr, dB.ptr, dC.ptr) == 0
        assert _delta(st0, eng.gemm_path_stats()) == {}
        out, gaps_ok = dC.read()
        assert gaps_ok and np.array_equal(out, c0)


@pytest.mark.parametrize("ca,cb", DTYPES, ids=DT_IDS)
def test_unit_extents_exact(eng, ca, cb):
    rng = np.random.default_rng(7)
    cc = ca or cb
    for (M, N, K) in ((1, 300, 40), (300, 1, 40), (200, 150, 1), (1, 1, 1), (1, 1, 3000)):
        a, b, c0 = _exact_inputs(rng, M, N, K, ca, cb)
        conj = (ca, cb)
        xr, xi = _int_product(a, b, conj)
        alpha, beta = ((2 - 1j), 0.5) if cc else (2.0, 0.5)
        ref = alpha * _as_float(xr, xi, cc) + beta * _as_float(*c0, cc)
        out, paths = _simple(eng, ca, cb, M, N, K, _as_float(*a, ca), _as_float(*b, cb), _as_float(*c0, cc),
                             alpha, beta, conj)
        assert paths.get("launches") == 1
        assert np.array_equal(out, ref), (M, N, K)


@pytest.mark.parametrize("ca,cb", DTYPES, ids=DT_IDS)
def test_beta_zero_ignores_nan_c(eng, ca, cb):
    """beta = 0 never reads C: a C full of NaN gives finite results, unsplit and split-K"""
    rng = np.random.default_rng(8)
    cc = ca or cb
    for (M, N, K), path in (((300, 200, 40), None), ((100, 90, 3000), "split_b1")):
        a, b, _ = _exact_inputs(rng, M, N, K, ca, cb)
        xr, xi = _int_product(a, b, (False, False))
        c0 = np.full((1, M, N), np.nan, np.complex128 if cc else np.float64)
        out, paths = _simple(eng, ca, cb, M, N, K, _as_float(*a, ca), _as_float(*b, cb), c0, -1.0, 0.0)
        if path:
            assert paths.get(path) == 1, paths
        assert np.all(np.isfinite(out))
        assert np.array_equal(out, -_as_float(xr, xi, cc))


@pytest.mark.parametrize("ca,cb", DTYPES[:3], ids=DT_IDS[:3])
def test_conj_on_real_operand_is_ignored(eng, ca, cb):
    rng = np.random.default_rng(9)
    cc = ca or cb
    for (M, N, K) in ((300, 200, 40), (100, 90, 3000)):
        a, b, c = _normal(rng, (1, M, K), ca), _normal(rng, (1, K, N), cb), _normal(rng, (1, M, N), cc)
        plain, _ = _simple(eng, ca, cb, M, N, K, a, b, c, 1.5, -0.5)
        conj = (not ca, not cb)          # conjugation asked for the real operand(s) only
        out, _ = _simple(eng, ca, cb, M, N, K, a, b, c, 1.5, -0.5, conj)
        assert np.array_equal(out, plain)


@pytest.mark.parametrize("ca,cb", DTYPES, ids=DT_IDS)
def test_subnormal_results_exact(eng, ca, cb):
    """integer operands times 2**-535: the exact products are integers times 2**-1070, subnormal - no flush to zero"""
    rng = np.random.default_rng(10)
    cc = ca or cb
    for (M, N, K) in ((300, 200, 40), (100, 90, 3000)):
        a, b, c0 = _exact_inputs(rng, M, N, K, ca, cb)
        xr, xi = _int_product(a, b, (ca, cb))
        assert max(np.abs(xr).max(), np.abs(xi).max()) < 2 ** 40
        def scaled(p, e, cplx):
            return _compose(np.ldexp(p[0].astype(np.float64), e), np.ldexp(p[1].astype(np.float64), e), cplx)
        sa, sb, sc = scaled(a, -535, ca), scaled(b, -535, cb), scaled(c0, -1070, cc)
        ref = scaled((xr + c0[0], xi + c0[1]), -1070, cc)
        out, _ = _simple(eng, ca, cb, M, N, K, sa, sb, sc, 1.0, 1.0, (ca, cb))
        tiny = np.abs(ref.real)
        assert np.any((tiny > 0) & (tiny < 2.0 ** -1022))
        bad = np.argwhere(out != ref)
        assert bad.size == 0, f"{len(bad)} of {out.size} subnormal results differ, first {bad[:3].tolist()}"


def test_refusals_leave_c_untouched(eng):
    """extents that disagree, a null operand and an unknown dtype are refused before anything is launched"""
    rng = np.random.default_rng(11)
    M, N, K = 40, 30, 20
    maps, sbs = layout("rowmajor", M, N, K, 1)
    dA = Placed(eng, _normal(rng, (1, M, K), True), maps[0], maps[1], 0, np.nan)
    dB = Placed(eng, _normal(rng, (1, K, N), True), maps[2], maps[3], 0, np.nan)
    c0 = _normal(rng, (1, M, N), True)
    dC = Placed(eng, c0, maps[4], maps[5], 0, C_FILL)
    bad_k = maps[:2] + (one(K + 1, N),) + maps[3:]
    bad_m = maps[:4] + (one(M + 1, N), maps[5])
    bad_n = maps[:5] + (one(N + 1, 1),)
    for m, pa, pc, dt, status in ((bad_k, dA.ptr, dC.ptr, None, E.MPSE_ERR_SHAPE),
                                  (bad_m, dA.ptr, dC.ptr, None, E.MPSE_ERR_SHAPE),
                                  (bad_n, dA.ptr, dC.ptr, None, E.MPSE_ERR_SHAPE),
                                  (maps, None, dC.ptr, None, E.MPSE_ERR_ARG),
                                  (maps, dA.ptr, None, None, E.MPSE_ERR_ARG),
                                  (maps, dA.ptr, dC.ptr, 7, E.MPSE_ERR_ARG)):
        st0 = eng.gemm_path_stats()
        st = _gemm(eng, True, True, (0, 0), m, 1, sbs, 1.0, 1.0, 0, pa, dB.ptr, pc, dtype_a=dt)
        assert st == status, (st, status)
        assert _delta(st0, eng.gemm_path_stats()) == {}
        out, gaps_ok = dC.read()
        assert gaps_ok and np.array_equal(out, c0)
