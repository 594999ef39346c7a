"""Shared pieces of tests/test_vector_gpu.py (the device against exact references) and tests/test_vector_refs_host.py
(a NumPy emulation of the device's summation order against the same references, on the CPU): the launch grids of the
vector kernels, the lengths at which those grids change, the input generators, the references and the error bounds.

The launch constants are repeated from the engine's sources on purpose (the tests must not read them back from the
engine): RED_THREADS, RED_MAX_BLOCKS and red_blocks() from renormalizer_amd/csrc/mpse_device.h, ew_blocks() from
renormalizer_amd/csrc/mpse_vec_kernels.h."""
import functools
import itertools
import math

import numpy as np

RED_THREADS = 256            # mpse_device.h
RED_MAX_BLOCKS = 512         # mpse_device.h
RED_DOUBLES_PER_THREAD = 2   # mpse_device.h red_blocks(): one workgroup per 512 doubles, up to the cap
EW_THREADS = 256             # mpse_vec_kernels.h ew_blocks(): 256 threads per block ...
EW_MAX_BLOCKS = 4096         # ... and at most 4096 blocks; beyond 1 048 576 elements a thread loops

U = 2.0 ** -53               # unit roundoff of float64

# lengths (elements) on both sides of every change of grid size, trip count and tail guard
REAL_RED_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 262143, 262144, 262145, 393217, 524289, 1000003)
CPLX_RED_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 130816, 130817, 131071, 131072, 131073, 262143, 262144, 262145,
                    393216, 393217, 1000003)
RMS_LENGTHS = (1, 255, 256, 257, 511, 512, 513, 262143, 262144, 262145, 300001)
EW_LENGTHS = (1, 255, 256, 257, 1048575, 1048576, 1048577, 2097157, 3145727)
RED_NMAX = 1000003
RMS_TOLS = ((1e-3, 1e-6), (0.0, 0.5), (1e-5, 0.0))       # (rtol, atol)


def red_lengths(cplx):
    return CPLX_RED_LENGTHS if cplx else REAL_RED_LENGTHS


def _ceil_div(a, b):
    return -(-a // b)


def red_grid(n_elems, doubles_per_elem):
    """(nb, stride, trips) of a two-stage reduction over n_elems elements whose grid is sized by
    n_elems * doubles_per_elem doubles: workgroups, elements between two trips of a thread, trips of the first thread."""
    nb = _ceil_div(n_elems * doubles_per_elem, RED_THREADS * RED_DOUBLES_PER_THREAD)
    nb = min(max(nb, 1), RED_MAX_BLOCKS)
    stride = nb * RED_THREADS
    return nb, stride, _ceil_div(n_elems, stride)


def dot_grid(n, cplx):
    """mpse_dotc / mpse_nrm2: the grid is sized in doubles (two per complex element)"""
    return red_grid(n, 2 if cplx else 1)


def rms_grid(n):
    """mpse_scaled_rms: the grid is sized in elements for both dtypes"""
    return red_grid(n, 1)


def ew_grid(n):
    nb = min(max(_ceil_div(n, EW_THREADS), 1), EW_MAX_BLOCKS)
    stride = nb * EW_THREADS
    return nb, stride, _ceil_div(n, stride)


# ------------------------------------------------------------------ bounds

# depth of the summation tree after a thread's own trips: 6 wave levels and 4 waves in the producer, the same again in
# k_reduce_final, plus its at most 2 sequential terms (26 leaves slack over 6 + 4 + 6 + 4 + 2)
TREE_DEPTH = 26


def dot_bound_factor(n, cplx):
    """|device - exact| <= factor * sum_i |terms_i| for one part of mpse_dotc: first-order worst case of the kernel's own
    summation tree, (P T + 26) roundings of 2^-53 with P products per element and part (1 real, 2 complex) and T trips
    per thread; the leading 2 is the margin for second-order terms and FMA contraction."""
    _, _, trips = dot_grid(n, cplx)
    return 2.0 * ((2 if cplx else 1) * trips + TREE_DEPTH) * U


def nrm2_bound_factor(n, cplx):
    """|device - sqrt(S)| <= factor * sqrt(S): the sum of squares S carries the relative error of dot_bound_factor (all
    terms positive), the square root halves it and adds one rounding; 3 more roundings for the double-precision
    reference sqrt(fsum) itself."""
    return 0.5 * dot_bound_factor(n, cplx) + 4.0 * U


def rms_bound_factor(n):
    """relative bound of mpse_scaled_rms: T trips and the tree for the sum of positive terms, and 7 roundings per term
    (two hypot, multiply, add, divide, square, and the final sqrt / mean), each allowed 1 ulp = 2 * 2^-53"""
    _, _, trips = rms_grid(n)
    return (trips + TREE_DEPTH + 2 * 7) * U


# ------------------------------------------------------------------ inputs

def _maybe_cplx(draw, n, cplx):
    return draw(n) + 1j * draw(n) if cplx else draw(n)


def f32_valued(rng, n, cplx):
    """float64 data with float32 values: every product of two entries is exact in double"""
    return _maybe_cplx(lambda k: rng.standard_normal(k).astype(np.float32).astype(np.float64), n, cplx)


def int_valued(rng, n, cplx):
    """integers in [-8, 8] (both parts): every partial sum of a dot product is an integer far below 2^53"""
    return _maybe_cplx(lambda k: rng.integers(-8, 9, k).astype(np.float64), n, cplx)


@functools.lru_cache(maxsize=None)
def dot_vectors(kind, cplx):
    """(x, y) of RED_NMAX elements, x != y; the tests use their leading n elements.  Do not modify."""
    rng = np.random.default_rng((17 if kind == "f32" else 29) + cplx)
    gen = f32_valued if kind == "f32" else int_valued
    x, y = gen(rng, RED_NMAX, cplx), gen(rng, RED_NMAX, cplx)
    assert not np.array_equal(x, y)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def cancelling_pair(cplx):
    """(x, y), float32 valued, RED_NMAX elements: y repeats the first half with the opposite sign against a shuffled copy of
    x, so the exact dot is that of the last element alone, about 1e-9 * sum |x_i| |y_i| in both parts."""
    rng = np.random.default_rng(41 + cplx)
    m = (RED_NMAX - 1) // 2
    a, b = f32_valued(rng, m, cplx), f32_valued(rng, m, cplx)
    perm = rng.permutation(m)
    s = float(np.float32(math.sqrt(1e-9 * np.abs(a * b).sum() * 2)))
    x = np.concatenate([a, a[perm], [s]])
    y = np.concatenate([b, -b[perm], [s * (1 + 1j) if cplx else s]])
    return x, y


def dot_terms(x, y):
    """(re_terms, im_terms): lists of arrays whose elements sum to Re / Im of sum conj(x) y; exact products for
    float32- and integer-valued input.  im_terms is empty for real input."""
    if np.iscomplexobj(x):
        return [x.real * y.real, x.imag * y.imag], [x.real * y.imag, -(x.imag * y.real)]
    return [x * y], []


def _fsum(arrays):
    return math.fsum(itertools.chain.from_iterable(a.tolist() for a in arrays))


def exact_dot(x, y):
    """((re, im), (sum |re terms|, sum |im terms|)): the correctly rounded exact dot product (math.fsum over exact
    products) and the sums of the terms' magnitudes that the bounds scale with"""
    re_t, im_t = dot_terms(x, y)
    return (_fsum(re_t), _fsum(im_t)), (_fsum([np.abs(t) for t in re_t]), _fsum([np.abs(t) for t in im_t]))


@functools.lru_cache(maxsize=None)
def dot_reference(kind, cplx, n, norm=False):
    """exact_dot of the leading n elements of dot_vectors(kind, cplx); norm=True: of x with itself"""
    x, y = dot_vectors(kind, cplx)
    return exact_dot(x[:n], x[:n] if norm else y[:n])


def rms_inputs(rng, n, cplx, away_from_zero):
    """(x, y1, y2): y1 dominates on about half of the elements and y2 on the others; with away_from_zero every part of
    y1 and y2 has magnitude >= 0.5 (for atol = 0)"""
    def draw(k):
        v = rng.standard_normal(k)
        return np.copysign(0.5 + np.abs(v), v) if away_from_zero else v
    x = _maybe_cplx(rng.standard_normal, n, cplx)
    y1, y2 = _maybe_cplx(draw, n, cplx), _maybe_cplx(draw, n, cplx)
    first = rng.random(n) < 0.5
    y1 = y1 * np.where(first, 4.0, 0.25)
    big1 = np.abs(y1) > np.abs(y2)
    assert n < 64 or (big1.any() and not big1.all())
    return x, y1, y2


def rms_overflow_inputs(rng, n):
    """complex x and y1 with components of +-1e200 (|x_i| = |y1_i|, a plain sqrt(re^2 + im^2) overflows), y2 small:
    with rtol = 1, atol = 0 the result is 1"""
    def draw():
        return 1e200 * (rng.choice([-1.0, 1.0], n) + 1j * rng.choice([-1.0, 1.0], n))
    return draw(), draw(), rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _abs_ld(v):
    if np.iscomplexobj(v):
        return np.hypot(v.real.astype(np.longdouble), v.imag.astype(np.longdouble))
    return np.abs(v.astype(np.longdouble))


def rms_reference(x, y1, y2, rtol, atol):
    """sqrt(mean((|x| / (atol + rtol max(|y1|, |y2|)))^2)) in np.longdouble"""
    ld = np.longdouble
    q = _abs_ld(x) / (ld(atol) + ld(rtol) * np.maximum(_abs_ld(y1), _abs_ld(y2)))
    return np.sqrt((q * q).sum() / ld(len(x)))


# ------------------------------------------------------------------ the device's summation order, in NumPy float64

def _block_tree(v):
    """(nb, 256) -> (nb,): 64 lanes of each wave pairwise (6 levels), then the 4 waves one after the other"""
    nb = v.shape[0]
    w = v.reshape(nb, RED_THREADS // 64, 64)
    while w.shape[2] > 1:
        w = w[:, :, 0::2] + w[:, :, 1::2]
    w = w[:, :, 0]
    s = np.zeros(nb)
    for i in range(w.shape[1]):
        s = s + w[:, i]
    return s


def two_stage_sum(term_rows, n, nb):
    """Sum n terms the way the reductions do: thread t of the grid (nb * 256 threads) adds its terms t, t + stride, ...
    in order, a fixed tree joins the 256 threads of a workgroup, and one workgroup joins the partials (each thread adds
    its partials t, t + 256 in order, then the same tree).  term_rows: arrays of n terms each; per trip a thread adds
    the rows' terms of its element one after the other."""
    stride = nb * RED_THREADS
    trips = _ceil_div(n, stride)
    acc = np.zeros(stride)
    for k in range(trips):
        lo, hi = k * stride, min(n, (k + 1) * stride)
        for row in term_rows:
            acc[:hi - lo] = acc[:hi - lo] + row[lo:hi]
    partial = _block_tree(acc.reshape(nb, RED_THREADS))
    pad = np.zeros(_ceil_div(nb, RED_THREADS) * RED_THREADS)
    pad[:nb] = partial
    fin = np.zeros(RED_THREADS)
    for k in range(len(pad) // RED_THREADS):
        fin = fin + pad[k * RED_THREADS:(k + 1) * RED_THREADS]
    return float(_block_tree(fin.reshape(1, RED_THREADS))[0])


def emulate_dot(x, y):
    """(re, im) of sum conj(x) y in the order of k_dot_partial + k_reduce_final.  The complex kernel adds the sum of an
    element's two products to its accumulator (one rounding for the pair, one for the accumulation)."""
    n = len(x)
    cplx = np.iscomplexobj(x)
    nb, _, _ = dot_grid(n, cplx)
    re_t, im_t = dot_terms(x, y)
    if not cplx:
        return two_stage_sum(re_t, n, nb), 0.0
    return two_stage_sum([re_t[0] + re_t[1]], n, nb), two_stage_sum([im_t[0] + im_t[1]], n, nb)


def emulate_scaled_rms(x, y1, y2, rtol, atol):
    n = len(x)
    nb, _, _ = rms_grid(n)

    def mag(v):
        return np.hypot(v.real, v.imag) if np.iscomplexobj(v) else np.abs(v)
    q = mag(x) / (atol + rtol * np.maximum(mag(y1), mag(y2)))
    return math.sqrt(two_stage_sum([q * q], n, nb) / float(n))
