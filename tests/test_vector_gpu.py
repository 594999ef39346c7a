"""The vector and data-movement entry points (mpse_vec.hip, mpse_vec_kernels.h, the gather kernels of mpse_qr.hip and the
transpose of mpse_gemm.hip) against exact or high-precision references at every length where their launch grids, trip
counts or tail guards change.  tests/test_vector_refs_host.py shows on the CPU that the summation order these constants
imply stays inside the bounds used here.  Run on the MI355X box: pytest -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest

from renormalizer_amd import engine as E
import vector_refs as vr            # (tests/vector_refs.py)

pytestmark = pytest.mark.gpu

# Launch constants, repeated from the sources (never read back from the engine):
RED_THREADS = 256            # renormalizer_amd/csrc/mpse_device.h
RED_MAX_BLOCKS = 512         # renormalizer_amd/csrc/mpse_device.h
RED_DOUBLES_PER_THREAD = 2   # red_blocks() of mpse_device.h: 512 doubles per workgroup up to the cap
EW_MAX_BLOCKS, EW_THREADS = 4096, 256     # ew_blocks() of renormalizer_amd/csrc/mpse_vec_kernels.h
assert (RED_THREADS, RED_MAX_BLOCKS, RED_DOUBLES_PER_THREAD, EW_MAX_BLOCKS, EW_THREADS) == \
    (vr.RED_THREADS, vr.RED_MAX_BLOCKS, vr.RED_DOUBLES_PER_THREAD, vr.EW_MAX_BLOCKS, vr.EW_THREADS)

U = 2.0 ** -53
OK, ERR_ARG = 0, 5           # include/mpsengine.h
PAD = 8                      # sentinel elements behind every output: a kernel must not write past n


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def _sub(t, start, n):
    """flat view of n elements of t from element ``start`` on"""
    return E.DeviceTensor(t.eng, t.buf, t.offset + int(start) * t.dtype.itemsize, (int(n),), t.dtype)


def _name(cplx):
    return "c128" if cplx else "f64"


def _dotc(eng, X, Y, n):
    out = (C.c_double * 2)(7.0, 7.0)
    assert eng.lib.mpse_dotc(eng.ctx, X.code, X.ptr, Y.ptr, n, out) == OK
    return out[0], out[1]


def _nrm2(eng, X, n):
    out = (C.c_double * 2)(7.0, 7.0)
    assert eng.lib.mpse_nrm2(eng.ctx, X.code, X.ptr, n, out) == OK
    assert out[1] == 7.0                    # one double of output
    return out[0]


# ------------------------------------------------------------------ reductions

@pytest.mark.parametrize("cplx", [False, True])
def test_dotc_nrm2_count_every_element_once(eng, cplx):
    """Integer entries in [-8, 8]: every partial sum is an integer below 2^53, so whatever the summation order the device
    must return the integer dot product exactly, in both parts - a skipped or doubled element or a wrong sign in the
    conjugation shows at the length where it happens."""
    x, y = vr.dot_vectors("int", cplx)
    X, Y = eng.asdevice(x), eng.asdevice(y)
    for n in vr.red_lengths(cplx):
        want = np.vdot(x[:n], y[:n])
        assert _dotc(eng, X, Y, n) == (want.real, want.imag), n
        assert _dotc(eng, Y, X, n) == (want.real, -want.imag), n
        sq = np.vdot(x[:n], x[:n]).real
        assert _dotc(eng, X, X, n) == (sq, 0.0), n
        assert _nrm2(eng, X, n) == math.sqrt(sq), n


@pytest.mark.parametrize("cplx", [False, True])
def test_dotc_nrm2_rounding(eng, cplx):
    """float32-valued data (exact products) against the correctly rounded exact sum (math.fsum):
    |err| <= 2 (P T + 26) 2^-53 sum |terms| per part, P products per element and part, T trips per thread; and one pair
    with heavy cancellation (exact dot ~ 1e-9 sum |x||y|) under the same bound."""
    x, y = vr.dot_vectors("f32", cplx)
    X, Y = eng.asdevice(x), eng.asdevice(y)
    worst_dot = worst_nrm = 0.0
    for n in vr.red_lengths(cplx):
        got = _dotc(eng, X, Y, n)
        ref, mags = vr.dot_reference("f32", cplx, n)
        f = vr.dot_bound_factor(n, cplx)
        for part, (g, r, m) in enumerate(zip(got, ref, mags)):
            if m == 0.0:
                assert g == 0.0, (n, part)
                continue
            ratio = abs(g - r) / (f * m)
            worst_dot = max(worst_dot, ratio)
            assert ratio <= 1.0, (n, part, g, r, ratio)
        (s_ref, _), _ = vr.dot_reference("f32", cplx, n, norm=True)
        ratio = abs(_nrm2(eng, X, n) - math.sqrt(s_ref)) / (vr.nrm2_bound_factor(n, cplx) * math.sqrt(s_ref))
        worst_nrm = max(worst_nrm, ratio)
        assert ratio <= 1.0, (n, ratio)
    print(f"mpse_dotc {_name(cplx)}: worst observed/bound = {worst_dot:.4f}")
    print(f"mpse_nrm2 {_name(cplx)}: worst observed/bound = {worst_nrm:.4f}")
    xc, yc = vr.cancelling_pair(cplx)
    n = len(xc)
    ref, mags = vr.exact_dot(xc, yc)
    got = _dotc(eng, eng.asdevice(xc), eng.asdevice(yc), n)
    worst = 0.0
    for g, r, m in zip(got, ref, mags):
        if m:
            assert abs(r) < 1e-8 * m
            worst = max(worst, abs(g - r) / (vr.dot_bound_factor(n, cplx) * m))
    print(f"mpse_dotc {_name(cplx)}, cancelling pair: observed/bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("cplx", [False, True])
def test_dotc_nrm2_consistency(eng, cplx):
    """norm()^2 against vdot(x, x).real (the square root rounds once, squaring it back doubles that and rounds again:
    3 * 2^-53 relative), Im vdot(x, x) within the rounding bound (the compiler may contract the products into FMA, so it
    need not be exactly 0), out_host[1] == 0 for real input, and two calls in a row bitwise equal."""
    rng = np.random.default_rng(61 + cplx)
    x = rng.standard_normal(vr.RED_NMAX) + (1j * rng.standard_normal(vr.RED_NMAX) if cplx else 0.0)
    y = rng.standard_normal(vr.RED_NMAX) + (1j * rng.standard_normal(vr.RED_NMAX) if cplx else 0.0)
    X, Y = eng.asdevice(x), eng.asdevice(y)
    worst_im = 0.0
    for n in vr.red_lengths(cplx):
        re, im = _dotc(eng, X, X, n)
        nrm = _nrm2(eng, X, n)
        assert abs(nrm * nrm - re) <= 3.0 * U * re * (1.0 + 8.0 * U), n
        if cplx:
            bound = vr.dot_bound_factor(n, cplx) * 2.0 * float(np.abs(x[:n].real * x[:n].imag).sum())
            assert abs(im) <= bound, (n, im, bound)
            worst_im = max(worst_im, abs(im) / bound)
        else:
            assert im == 0.0, n
        first = _dotc(eng, X, Y, n)
        assert _dotc(eng, X, Y, n) == first, n
        if not cplx:
            assert first[1] == 0.0, n
        assert _nrm2(eng, X, n) == nrm, n
    v, w = _sub(X, 0, 1000), _sub(Y, 0, 1000)                   # the Python wrappers are the same calls
    re, im = _dotc(eng, X, Y, 1000)
    assert v.vdot(w) == (complex(re, im) if cplx else re) and v.norm() == _nrm2(eng, X, 1000)
    if cplx:
        print(f"Im mpse_dotc(x, x) c128: worst observed/bound = {worst_im:.4f}")


def _scaled_rms(eng, X, Y1, Y2, n, rtol, atol):
    out = (C.c_double * 2)(7.0, 7.0)
    assert eng.lib.mpse_scaled_rms(eng.ctx, X.code, X.ptr, Y1.ptr, Y2.ptr, n, rtol, atol, out) == OK
    assert out[1] == 7.0
    return out[0]


@pytest.mark.parametrize("cplx", [False, True])
def test_scaled_rms(eng, cplx):
    """Against sqrt(mean((|x| / (atol + rtol max(|y1|, |y2|)))^2)) in np.longdouble, y1 larger on some elements and y2
    on others.  All terms are positive, so the bound is relative: (T + 26 + 2 * 7) 2^-53 - T trips and the tree for the
    sum, 7 roundings per term (two hypot, multiply, add, divide, square, and the final sqrt / mean) of 1 ulp each."""
    rng = np.random.default_rng(53 + cplx)
    worst = 0.0
    for n in vr.RMS_LENGTHS:
        for rtol, atol in vr.RMS_TOLS:
            x, y1, y2 = vr.rms_inputs(rng, n, cplx, away_from_zero=(atol == 0.0))
            ref = vr.rms_reference(x, y1, y2, rtol, atol)
            X, Y1, Y2 = eng.asdevice(x), eng.asdevice(y1), eng.asdevice(y2)
            got = _scaled_rms(eng, X, Y1, Y2, n, rtol, atol)
            ratio = abs(float((np.longdouble(got) - ref) / ref)) / vr.rms_bound_factor(n)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (n, rtol, atol, got, float(ref), ratio)
            assert _scaled_rms(eng, X, Y1, Y2, n, rtol, atol) == got
    print(f"mpse_scaled_rms {_name(cplx)}: worst observed/bound = {worst:.4f}")


def test_scaled_rms_components_of_1e200(eng):
    """|x_i| = |y1_i| with components of +-1e200, rtol = 1, atol = 0: a plain sqrt(re^2 + im^2) would overflow; the result
    is 1 within the bound"""
    rng = np.random.default_rng(59)
    for n in (513, 262145):
        x, y1, y2 = vr.rms_overflow_inputs(rng, n)
        got = _scaled_rms(eng, eng.asdevice(x), eng.asdevice(y1), eng.asdevice(y2), n, 1.0, 0.0)
        print(f"mpse_scaled_rms c128, components of 1e200, n = {n}: |result - 1| / bound = "
              f"{abs(got - 1.0) / vr.rms_bound_factor(n):.4f}")
        assert abs(got - 1.0) <= vr.rms_bound_factor(n), (n, got)


# ------------------------------------------------------------------ elementwise kernels

EW_NMAX = vr.EW_LENGTHS[-1]
EW_ALLOC = EW_NMAX + PAD + 1              # (+1: the real views that start one element into their buffer)


@pytest.fixture(scope="module")
def ew(eng):
    """host vectors and their device copies, shared by the elementwise tests (never modified), and two work buffers"""
    rng = np.random.default_rng(71)
    h = {k: rng.standard_normal(EW_ALLOC) for k in ("xr", "yr", "m")}
    h["xc"] = rng.standard_normal(EW_ALLOC) + 1j * rng.standard_normal(EW_ALLOC)
    h["yc"] = rng.standard_normal(EW_ALLOC) + 1j * rng.standard_normal(EW_ALLOC)
    for a in h.values():
        a.setflags(write=False)
    d = {k: eng.asdevice(a) for k, a in h.items()}
    d["wr"], d["wc"] = eng.empty((EW_ALLOC,), np.float64), eng.empty((EW_ALLOC,), np.complex128)
    return h, d


def _run(eng, ew, cplx_out, init, n, shift, launch):
    """work[shift : shift + n + PAD] = init[shift : ...]; launch(view of n elements at ``shift``); returns the n results
    after checking that the PAD elements behind them still hold what was there."""
    h, d = ew
    work = d["wc" if cplx_out else "wr"]
    src = _sub(d[init], shift, n + PAD)
    dst = _sub(work, shift, n + PAD)
    eng._check(eng.lib.mpse_memcpy_d2d(eng.ctx, dst.ptr, src.ptr, dst.nbytes))
    assert launch(_sub(work, shift, n)) == OK
    res = dst.to_host()
    assert np.array_equal(res[n:], h[init][shift + n:shift + n + PAD]), ("wrote past n", n, shift)
    return res[:n]


def _shifts(cplx):
    return (0,) if cplx else (0, 1)         # a real view may start 8 bytes into its buffer; complex data is 16-byte aligned


def test_cast_conj_real_part_bitwise(eng, ew):
    h, d = ew
    lib, ctx = eng.lib, eng.ctx
    for n in vr.EW_LENGTHS:
        for s in (0, 1):
            xs = _sub(d["xr"], s, n)
            got = _run(eng, ew, True, "yc", n, 0, lambda w: lib.mpse_cast_f64_to_c128(ctx, w.ptr, xs.ptr, n))
            assert np.array_equal(got, h["xr"][s:s + n].astype(np.complex128)), ("cast", n, s)
            got = _run(eng, ew, False, "yr", n, s, lambda w: lib.mpse_real_part(ctx, w.ptr, d["xc"].ptr, n))
            assert np.array_equal(got, h["xc"][:n].real), ("real_part", n, s)
        got = _run(eng, ew, True, "xc", n, 0, lambda w: lib.mpse_conj_inplace(ctx, w.ptr, n))
        assert np.array_equal(got, h["xc"][:n].conj()), ("conj", n)
        assert np.array_equal(np.signbit(got.imag), ~np.signbit(h["xc"][:n].imag)), ("conj", n)


@pytest.mark.parametrize("cplx", [False, True])
def test_mul_real_bitwise(eng, ew, cplx):
    h, d = ew
    key = "xc" if cplx else "xr"
    for n in vr.EW_LENGTHS:
        for s in _shifts(cplx):
            for ms in (0, 1):                                   # the weights are real: aligned and 8 bytes in
                m = _sub(d["m"], ms, n)
                got = _run(eng, ew, cplx, key, n, s, lambda w: eng.lib.mpse_mul_real(eng.ctx, w.code, w.ptr, m.ptr, n))
                x, mh = h[key][s:s + n], h["m"][ms:ms + n]
                want = (x.real * mh + 1j * (x.imag * mh)) if cplx else x * mh
                assert np.array_equal(got, want), (n, s, ms)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _check_axpy_like(got, a, x, y, what):
    """got = y + a x per component within 3 * 2^-53 (|y| + |a_re x_re| + |a_im x_im|) (y = None: a x), against the
    same expression in np.longdouble (its own error, 2^-64 relative, is 2^-11 of the bound).  Returns the worst
    observed / bound."""
    a = complex(a)
    xr, xi = _ld(x.real), _ld(x.imag)
    parts = [(xr * a.real, -(xi * a.imag), got.real, None if y is None else y.real)]
    if np.iscomplexobj(x):
        parts.append((xi * a.real, xr * a.imag, got.imag, None if y is None else y.imag))
    worst = 0.0
    for p1, p2, g, y0 in parts:
        ref, mag = p1 + p2, np.abs(p1) + np.abs(p2)
        if y0 is not None:
            ref, mag = ref + _ld(y0), mag + np.abs(_ld(y0))
        ratio = np.abs(_ld(g) - ref) / (3.0 * U * mag)
        worst = max(worst, float(ratio.max()))
        assert worst <= 1.0, (what, int(ratio.argmax()), worst)
    return worst


@pytest.mark.parametrize("cplx", [False, True])
def test_scal(eng, ew, cplx):
    """real: one rounding, bitwise equal to NumPy; complex: per component |err| <= 3 * 2^-53 (|a_re v_re| + |a_im v_im|)"""
    h, d = ew
    key = "xc" if cplx else "xr"
    a = (0.3 - 1.2j) if cplx else -0.7
    worst = 0.0
    for n in vr.EW_LENGTHS:
        for s in _shifts(cplx):
            got = _run(eng, ew, cplx, key, n, s,
                       lambda w: eng.lib.mpse_scal(eng.ctx, w.code, w.ptr, n, complex(a).real, complex(a).imag))
            x = h[key][s:s + n]
            if cplx:
                worst = max(worst, _check_axpy_like(got, a, x, None, ("scal", n)))
            else:
                assert np.array_equal(got, x * a), (n, s)
    if cplx:
        print(f"mpse_scal c128: worst observed/bound = {worst:.4f}")
    else:
        # the real kernel never reads the imaginary part of the factor
        got = _run(eng, ew, False, key, 257, 0, lambda w: eng.lib.mpse_scal(eng.ctx, w.code, w.ptr, 257, a, 123.0))
        assert np.array_equal(got, h[key][:257] * a)


@pytest.mark.parametrize("cplx", [False, True])
def test_axpy(eng, ew, cplx):
    """y += a x per component within 3 * 2^-53 (|y| + |a_re x_re| + |a_im x_im|)"""
    h, d = ew
    kx, ky = ("xc", "yc") if cplx else ("xr", "yr")
    a = complex(0.3, -1.2) if cplx else complex(-0.7, 0.0)
    worst = 0.0
    for n in vr.EW_LENGTHS:
        for s in _shifts(cplx):
            xs = 0 if cplx else 1 - s                           # x and y at different alignments
            xv = _sub(d[kx], xs, n)
            got = _run(eng, ew, cplx, ky, n, s,
                       lambda w: eng.lib.mpse_axpy(eng.ctx, w.code, w.ptr, xv.ptr, n, a.real, a.imag))
            worst = max(worst, _check_axpy_like(got, a, h[kx][xs:xs + n], h[ky][s:s + n], ("axpy", n, s)))
    print(f"mpse_axpy {_name(cplx)}: worst observed/bound = {worst:.4f}")


# ------------------------------------------------------------------ gathers and the transpose

def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _pdbl(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _scaled(a, scale, axis):
    """a * scale along ``axis`` with one rounding per component (complex: both parts by the real factor)"""
    if scale is None:
        return a
    s = scale[:, None] if axis == 0 else scale[None, :]
    return (a.real * s + 1j * (a.imag * s)) if np.iscomplexobj(a) else a * s


def _index_lists(rng, n_in, n_out):
    """a permutation, a strict subset, repeated indices, a single index - all in range"""
    lists = [rng.permutation(n_in)[:1]]
    if n_in > 1:
        lists.append(rng.permutation(n_in))
        lists.append(np.sort(rng.permutation(n_in)[:n_out])[::-1].copy())
        rep = rng.integers(0, n_in, n_out)
        rep[-1] = rep[0]
        lists.append(rep)
    return [np.ascontiguousarray(i, dtype=np.int64) for i in lists]


def _out_with_sentinel(eng, n, dtype):
    out = eng.empty((n + PAD,), dtype)
    tail = np.full(PAD, -777.0, dtype=dtype)
    eng._check(eng.lib.mpse_memcpy_h2d(eng.ctx, _sub(out, n, PAD).ptr, tail.ctypes.data, tail.nbytes))
    return out, tail


@pytest.mark.parametrize("cplx", [False, True])
def test_gather_cols_and_rows_bitwise(eng, cplx):
    """out[:, j] = in[:, cols[j]] * scale[j] and out[i, :] = in[rows[i], :] * scale[i], bitwise, with and without the
    scale; (1100, 1000) -> 960 columns and 960 rows of (1000, 1100) have more elements than the capped grid has threads."""
    rng = np.random.default_rng(83 + cplx)
    dt = np.complex128 if cplx else np.float64
    for (nrow, ncol, nsel, axis) in [(1, 1, 1, 1), (3, 257, 5, 1), (1100, 1000, 960, 1),
                                     (1, 1, 1, 0), (257, 3, 5, 0), (1000, 1100, 960, 0)]:
        a = rng.standard_normal((nrow, ncol)) + (1j * rng.standard_normal((nrow, ncol)) if cplx else 0.0)
        A = eng.asdevice(a)
        n_in = ncol if axis == 1 else nrow
        for idx in _index_lists(rng, n_in, nsel):
            assert idx.min() >= 0 and idx.max() < n_in
            for scale in (None, rng.uniform(0.5, 2.0, len(idx)) * rng.choice([-1.0, 1.0], len(idx))):
                k = len(idx)
                total = nrow * k if axis == 1 else k * ncol
                out, tail = _out_with_sentinel(eng, total, dt)
                if axis == 1:
                    st = eng.lib.mpse_gather_cols(eng.ctx, A.code, out.ptr, A.ptr, nrow, ncol, _p64(idx), _pdbl(scale), k)
                    want = _scaled(a[:, idx], scale, 1)
                else:
                    st = eng.lib.mpse_gather_rows(eng.ctx, A.code, out.ptr, A.ptr, ncol, _p64(idx), _pdbl(scale), k)
                    want = _scaled(a[idx, :], scale, 0)
                assert st == OK
                res = out.to_host()
                assert np.array_equal(res[:total].reshape(want.shape), want), (nrow, ncol, axis, k, scale is None)
                assert np.array_equal(res[total:], tail), "wrote past the output"


@pytest.mark.parametrize("cplx", [False, True])
def test_transpose_inner_shapes_bitwise(eng, cplx):
    """(d0, d1, d2) -> (d0, d2, d1) through 32 x 32 tiles: extents of one, below, at and above the tile, several tiles
    per plane; conj = 1 conjugates complex data and leaves real data alone"""
    rng = np.random.default_rng(89 + cplx)
    dt = np.complex128 if cplx else np.float64
    for shape in [(1, 1, 1), (2, 31, 33), (3, 32, 32), (1, 33, 1), (1, 1, 65), (5, 64, 96), (2, 100, 7)]:
        a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0.0)
        A = eng.asdevice(a)
        for conj in (0, 1):
            out, tail = _out_with_sentinel(eng, a.size, dt)
            assert eng.lib.mpse_transpose_inner(eng.ctx, A.code, out.ptr, A.ptr, *shape, conj) == OK
            want = a.transpose(0, 2, 1)
            if conj and cplx:
                want = want.conj()
            res = out.to_host()
            assert np.array_equal(res[:a.size].reshape(want.shape), want), (shape, conj)
            if cplx:
                assert np.array_equal(np.signbit(res[:a.size].imag.reshape(want.shape)), np.signbit(want.imag))
            assert np.array_equal(res[a.size:], tail), "wrote past the output"


# ------------------------------------------------------------------ argument contract

def _calls(eng, bufs, n, out_host):
    """every entry point of this file as (name, call(ptrs...), number of device operands); operand 0 is the output"""
    lib, ctx = eng.lib, eng.ctx
    idx = np.arange(max(n, 1), dtype=np.int64)
    one = np.ones(max(n, 1))
    calls = []
    for code, name in ((E.F64, "f64"), (E.C128, "c128")):
        calls += [
            (f"scal {name}", lambda x, c=code: lib.mpse_scal(ctx, c, x, n, 0.5, 0.0), 1),
            (f"axpy {name}", lambda y, x, c=code: lib.mpse_axpy(ctx, c, y, x, n, 0.5, 0.0), 2),
            (f"mul_real {name}", lambda x, m, c=code: lib.mpse_mul_real(ctx, c, x, m, n), 2),
            (f"dotc {name}", lambda x, y, c=code: lib.mpse_dotc(ctx, c, x, y, n, out_host), 2),
            (f"nrm2 {name}", lambda x, c=code: lib.mpse_nrm2(ctx, c, x, n, out_host), 1),
            (f"scaled_rms {name}", lambda x, y1, y2, c=code: lib.mpse_scaled_rms(ctx, c, x, y1, y2, n, 1e-3, 1e-6,
                                                                               out_host), 3),
            (f"gather_cols {name}", lambda o, i, c=code: lib.mpse_gather_cols(ctx, c, o, i, 1, n, _p64(idx), _pdbl(one),
                                                                            n), 2),
            (f"gather_rows {name}", lambda o, i, c=code: lib.mpse_gather_rows(ctx, c, o, i, 1, _p64(idx), _pdbl(one), n),
             2),
            (f"transpose_inner {name}", lambda o, i, c=code: lib.mpse_transpose_inner(ctx, c, o, i, 1, n, 1, 0), 2),
        ]
    calls += [
        ("cast", lambda dst, src: lib.mpse_cast_f64_to_c128(ctx, dst, src, n), 2),
        ("conj", lambda x: lib.mpse_conj_inplace(ctx, x, n), 1),
        ("real_part", lambda o, z: lib.mpse_real_part(ctx, o, z, n), 2),
    ]
    return calls


def test_zero_length_calls_touch_nothing(eng):
    """n = 0: MPSE_OK, the buffers keep their contents, and a pre-filled out_host is zeroed"""
    vals = np.arange(1.0, 9.0) + 1j * np.arange(11.0, 19.0)
    bufs = [eng.asdevice(vals) for _ in range(3)]
    out_host = (C.c_double * 2)(7.0, 7.0)
    for name, call, nops in _calls(eng, bufs, 0, out_host):
        out_host[0] = out_host[1] = 7.0
        assert call(*[b.ptr for b in bufs[:nops]]) == OK, name
        for b in bufs:
            assert np.array_equal(b.to_host(), vals), name
        if name.startswith("dotc"):
            assert (out_host[0], out_host[1]) == (0.0, 0.0), name
        elif name.startswith(("nrm2", "scaled_rms")):
            assert out_host[0] == 0.0, name
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert eng.lib.mpse_transpose_inner(eng.ctx, E.C128, bufs[0].ptr, bufs[1].ptr, *dims, 1) == OK
    idx = np.zeros(1, dtype=np.int64)
    assert eng.lib.mpse_gather_cols(eng.ctx, E.C128, bufs[0].ptr, bufs[1].ptr, 0, 4, _p64(idx), None, 1) == OK
    assert eng.lib.mpse_gather_rows(eng.ctx, E.C128, bufs[0].ptr, bufs[1].ptr, 0, _p64(idx), None, 1) == OK
    assert np.array_equal(bufs[0].to_host(), vals)


def test_null_operands_are_refused(eng):
    """a NULL operand with n > 0: MPSE_ERR_ARG, nothing launched, nothing written"""
    n = 4
    vals = np.arange(1.0, 9.0) + 1j * np.arange(11.0, 19.0)
    bufs = [eng.asdevice(vals) for _ in range(3)]
    out_host = (C.c_double * 2)(7.0, 7.0)
    for name, call, nops in _calls(eng, bufs, n, out_host):
        for null in range(nops):
            ptrs = [None if i == null else bufs[i].ptr for i in range(nops)]
            assert call(*ptrs) == ERR_ARG, (name, null)
    lib, ctx = eng.lib, eng.ctx
    x, y = bufs[0].ptr, bufs[1].ptr
    assert lib.mpse_dotc(ctx, E.F64, x, y, n, None) == ERR_ARG
    assert lib.mpse_nrm2(ctx, E.F64, x, n, None) == ERR_ARG
    assert lib.mpse_scaled_rms(ctx, E.F64, x, y, y, n, 1e-3, 1e-6, None) == ERR_ARG
    assert lib.mpse_gather_cols(ctx, E.F64, x, y, 1, n, None, None, n) == ERR_ARG
    assert lib.mpse_gather_rows(ctx, E.F64, x, y, 1, None, None, n) == ERR_ARG
    for b in bufs:
        assert np.array_equal(b.to_host(), vals)
