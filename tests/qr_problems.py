"""Constructed blocks for the Cholesky-QR kernels of mpse_block_qr (mpse_cholqr.hip), with a float64 emulation of the
rule by which the device decides, per block, how to factorise them (tests/test_block_qr_chol_gpu.py asserts the
decisions from mpse_block_qr_path_stats; tests/test_qr_problems_host.py holds every case to the margins below).

The device rule (constants of cholqr_run, k_cq_chol / k_cq_chol_rl and panel_eliminate):
  pass 1   G = A^H A; Cholesky of G in which a pivot that has lost all but THETA of its diagonal entry
           (d_k <= THETA G_kk) counts as d_k + s, s = 11 (m n + n (n + 1)) u trace(G); A1 = A R1^-1
  pass 2   G2 = A1^H A1, dev2 = n max|G2 - I| (the larger of the real and the imaginary part, entry by entry);
           dev2 <= FIRST_ORDER: R2 = I + striu(E) + diag(E) / 2, E = G2 - I, and A2 = A1 - A1 (R2 - I); otherwise the
           plain Cholesky factor and a triangular solve.  dev2 <= TAU: the block is done after this pass
  pass 3   the same with G3 = A2^H A2 for the blocks that are not done
  the pivots of a block's LAST pass must lie in WINDOW, those of every pass must be positive: otherwise the call is
  redone by the Householder kernels.

Four decision classes, each far from the thresholds (what decides is the condition number of the block, for I and II
after scaling its columns to unit norm):
  I    orthonormal columns ("I"), and orthonormal columns scaled by logspace(0, -9, n) ("Is"):
       no pivot shifted, first-order factor at pass 2, two passes
  II   geometric spectrum, kappa = 1e5: no pivot shifted, plain factor at pass 2, two passes
  III  geometric spectrum, kappa = 1e8: shifted pivots, three passes, first-order factor at pass 3
  IV   geometric spectrum, kappa = 1e12: shifted pivots, three passes, plain factor at pass 3 inside the pivot window
(kappa = 1e7 comes within a factor 5 of TAU, 1e10 straddles FIRST_ORDER at pass 3, 1e13 may break down: not usable.)

Smallest margin over every case of ``single_cases()`` and ``MIXED`` as emulated by tests/test_qr_problems_host.py - the
factor by which dev2 / dev3 stay away from FIRST_ORDER and TAU on the side the class claims: see MARGIN_MEASURED below;
the host test asserts >= MARGIN for every case.
"""
import zlib

import numpy as np

THETA, TAU, FIRST_ORDER, WINDOW = 1e-12, 0.1, 1e-9, (0.25, 4.0)
UNIT = 2.0 ** -53
RL_MAX_COLS, MAX_COLS = 160, 256      # right-looking factor kernel up to here / Cholesky-QR up to here
RPC = 32                              # rows per chunk of the Gram product for every height used here (see chunks())
MARGIN = 100.0
# smallest margins measured by the host test over all cases (real and complex; it prints the table with -s):
#   class I    1.6e3 below FIRST_ORDER (Is, 256 x 256), no pivot of pass 1 below its diagonal entry to rounding
#   class II   4.2e2 above FIRST_ORDER (16 x 16), 5.8e3 below TAU (176 x 176), pivot ratio 4.1e3 above THETA
#   class III  1.46e2 above TAU (15 x 15), 3.2e2 below FIRST_ORDER (257 x 255)
#   class IV   1.50e2 above TAU (17 x 15), 3.0e2 above FIRST_ORDER (18 x 17)
# (above TAU the margin is 10 n max|G2 - I| with max|G2 - I| = 0.97 ... 1: a shifted pivot leaves a diagonal entry of G2
# near zero, whatever the rounding.)  The smallest of all - the host test asserts that it measures this figure to 10 %:
MARGIN_MEASURED = 145.7

CLASSES = ("I", "Is", "II", "III", "IV")
KAPPA = {"II": 1e5, "III": 1e8, "IV": 1e12}
# per class: (pivots shifted in pass 1, passes, last factor is the first-order one)
CLAIMS = {"I": (False, 2, True), "Is": (False, 2, True), "II": (False, 2, False), "III": (True, 3, True),
          "IV": (True, 3, False)}
STAT_NAMES = ("chol_calls", "right_looking", "left_looking", "fallbacks", "blocks", "two_pass", "first_order_pass2",
              "first_order_pass3")

WIDTHS = (1, 15, 16, 17, 32, 33, 145, 160, 161, 176, 255, 256)
# the third height of every width: 5, 6 or 7 row chunks of 32 rows (two macro chunks of four waves, the second ragged)
# and no multiple of 16 (a ragged last workgroup of k_cq_trsm).  A block is at least as tall as wide, so 255 and 256
# columns cannot have fewer than 8 chunks: 21 and 22 chunks there (six macro chunks, the last ragged)
TALL = {1: 130, 15: 170, 16: 200, 17: 150, 32: 185, 33: 210, 145: 155, 160: 190, 161: 220, 176: 203, 255: 650, 256: 700}


def heights(n):
    """(square, one row more - two when that is a multiple of 4 -, the tall height of TALL) for a block of n columns:
    at RPC = 32 rows per chunk the first two give ceil(n / 32) chunks (9 for 255 and 256 columns with 257 rows: one row
    in the last), the last chunk partly filled unless n is 32, 160 or 256 and the block square"""
    m = n + 1
    if m % 4 == 0:
        m += 1
    return n, m, TALL[n]


def chunks(m, n_cu=256, groups=1):
    """(row chunks, rows per chunk) of a block of m rows by the rule of cholqr_run: about 8 waves per compute unit over
    the ``groups`` 2 x 2 super-tiles of all blocks of the call, at least 32 rows and at most 64 chunks"""
    want = min(64, max(1, -(-8 * n_cu // groups)))
    rpc = (max(32, -(-m // want)) + 3) & ~3
    return -(-m // rpc), rpc


def super_tiles(widths):
    return sum((p2 * (p2 + 1)) // 2 for p2 in (((w + 15) // 16 + 1) // 2 for w in widths))


def classes_of(n):
    """the classes a block of n columns is tested in: one column has no condition number"""
    return ("I",) if n == 1 else CLASSES


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def spectrum(cls, n):
    """the singular values the block is built with, descending"""
    if cls == "I":
        return np.ones(n)
    if cls == "Is":
        return np.logspace(0, -9, n)
    return np.logspace(0, -np.log10(KAPPA[cls]), n)


# Cases that were drawn again, with this suffix to the seed's key (the first suffix in alphabetical order that meets
# the condition).  The first three missed MARGIN itself (class IV at 16 and 17 columns: the pass-3 deviation of single
# draws scatters over three decades).  The others met it with less than a factor 3 to spare in a deviation that is
# amplified rounding error (class II at pass 2, classes III and IV at pass 3) and so may move with the BLAS that runs
# the emulation: every such margin is now >= 300, while the host test goes on asserting MARGIN.
REDRAWN = {"IV/200/16/1": "/b", "IV/17/16/0": "/c", "IV/18/17/0": "/b",
           "II/15/15/1": "/b", "III/257/255/1": "/b", "II/15/15/0": "/b", "IV/200/16/0": "/b", "IV/33/33/0": "/b",
           "III/176/176/0": "/b", "III/257/256/0": "/d"}


def block(cls, m, n, cplx):
    """The m x n block of class ``cls``: U diag(s) V^H with random orthonormal U (m x n) and V, s = spectrum(cls, n);
    class Is is U diag(s) - orthonormal columns scaled column-wise, its singular values are s again.  The same block for
    the same arguments (the seed is derived from them)."""
    key = f"{cls}/{m}/{n}/{int(cplx)}"
    rng = np.random.default_rng(zlib.crc32((key + REDRAWN.get(key, "")).encode()))
    u, _, vh = np.linalg.svd(_rand(rng, (m, n), cplx), full_matrices=False)
    s = spectrum(cls, n)
    return u * s if cls == "Is" else (u * s) @ vh


# ---------------------------------------------------------------------------------------------------------- emulator

def _cholesky(g, thr=None, shift=0.0):
    """(R, pivots as used, pivots before the shift): right-looking Cholesky R^H R = G (+ D) with the pivot rule of
    panel_eliminate: a pivot d_k <= thr[k] counts as d_k + shift.  A non-positive pivot is returned as it is (the
    device flags it); the factor is meaningless from there on."""
    n = g.shape[0]
    s = np.array(g, dtype=g.dtype)
    r = np.zeros_like(s)
    piv, raw = np.zeros(n), np.zeros(n)
    for k in range(n):
        d = raw[k] = s[k, k].real
        if thr is not None and not d > thr[k]:
            d += shift
        piv[k] = d
        if not d > 0.0:
            return r, piv, raw
        row = s[k, k:].copy()
        row[0] = d
        r[k, k:] = row / np.sqrt(d)
        s[k + 1:, k + 1:] -= np.outer(row[1:].conj(), row[1:]) / d
    return r, piv, raw


def _dev(g):
    """n max|G - I| as k_cq_reduce forms it: per entry the larger of |real| and |imaginary|"""
    e = g - np.eye(g.shape[0])
    return g.shape[0] * float(max(np.abs(e.real).max(), np.abs(e.imag).max()))


def _solve(a, r):
    """A R^-1 by substitution (backward stable, as k_cq_trsm)"""
    from scipy.linalg import solve_triangular
    return solve_triangular(r, a.conj().T, trans="C", lower=False).conj().T


def _factor_pass(a, n):
    """One of passes 2 and 3: (A R^-1, dev, first-order factor taken, pivots - None for the first-order factor)"""
    g = a.conj().T @ a
    dev = _dev(g)
    if dev <= FIRST_ORDER:
        e = g - np.eye(n)
        u = np.triu(e, 1) + np.diag(np.diag(e).real) / 2
        return a - a @ u, dev, True, None
    r, piv, _ = _cholesky(g)
    return (_solve(a, r) if piv.min() > 0 else a), dev, False, piv


def emulate(a, theta=THETA, tau=TAU):
    """What the device rule decides for the block ``a`` (m x n, m >= n), in float64 like the kernels:
    dict(shifted = pivots shifted in pass 1, pivot_ratio = min d_k / G_kk of pass 1 before the shift, dev2, dev3 (None
    after two passes), passes, first_order = the last factor is the first-order one, pivots = those of the last pass
    (None for a first-order factor), positive = every pivot of every pass was positive, orth = max|Q^H Q - I| of the
    emulated result)."""
    assert (theta, tau) == (THETA, TAU), "the emulator knows the defaults of MPSE_CHOLQR_THETA / MPSE_CHOLQR_TAU only"
    a = np.asarray(a)
    m, n = a.shape
    g = a.conj().T @ a
    diag = np.diag(g).real
    shift = 11.0 * (float(m) * n + float(n) * (n + 1)) * UNIT * float(diag.sum())
    r1, piv1, raw1 = _cholesky(g, theta * diag, shift)
    out = {"shifted": int((piv1 != raw1).sum()), "pivot_ratio": float((raw1 / np.where(diag > 0, diag, 1.0)).min()), "dev3": None}
    positive = bool(piv1.min() > 0)
    a1 = _solve(a, r1)
    a2, out["dev2"], fo, piv = _factor_pass(a1, n)
    out["passes"] = 2 if out["dev2"] <= tau else 3
    if piv is not None:
        positive = positive and bool(piv.min() > 0)
    q = a2
    if out["passes"] == 3:
        q, out["dev3"], fo, piv = _factor_pass(a2, n)
        if piv is not None:
            positive = positive and bool(piv.min() > 0)
    out["first_order"], out["pivots"], out["positive"] = fo, piv, positive
    out["orth"] = float(np.abs(q.conj().T @ q - np.eye(n)).max())
    return out


def margins(cls, em):
    """The factors by which the emulated quantities of a block stay on the side its class claims: every entry must be
    >= MARGIN.  A decision the emulation does not share gives a margin below 1."""
    _, passes, first = CLAIMS[cls]
    out = {}
    if passes == 2:
        out["dev2 below tau"] = TAU / max(em["dev2"], 1e-300)
        last = em["dev2"]
    else:
        out["dev2 above tau"] = em["dev2"] / TAU
        last = em["dev3"] if em["dev3"] is not None else np.inf
    if first:
        out["last dev below first-order"] = FIRST_ORDER / max(last, 1e-300)
    else:
        out["last dev above first-order"] = last / FIRST_ORDER
    return out


def predict(widths, classes):
    """The change of mpse_block_qr_path_stats over ONE call whose blocks have these widths and classes (no fallback)"""
    claims = [CLAIMS[c] for c in classes]
    rl = max(widths) <= RL_MAX_COLS
    return dict(zip(STAT_NAMES, (1, int(rl), int(not rl), 0, len(widths),
                                 sum(p == 2 for _, p, _ in claims), sum(p == 2 and f for _, p, f in claims),
                                 sum(p == 3 and f for _, p, f in claims))))


NO_CHANGE = dict.fromkeys(STAT_NAMES, 0)


# ----------------------------------------------------------------------------------------------------------- layouts

def layout(shapes, seed):
    """[(rows, cols)]: the blocks of one call, block b with shapes[b] = (m, n) rows and columns of a sum(m) x sum(n)
    matrix, rows and columns of all blocks interleaved by a random permutation (index lists ascending inside a block)"""
    rng = np.random.default_rng(seed)
    ms, ns = [s[0] for s in shapes], [s[1] for s in shapes]
    pr, pc = rng.permutation(sum(ms)), rng.permutation(sum(ns))
    ro, co = np.cumsum([0] + ms), np.cumsum([0] + ns)
    return [(np.sort(pr[ro[b]:ro[b + 1]]).astype(np.int64), np.sort(pc[co[b]:co[b + 1]]).astype(np.int64))
            for b in range(len(shapes))]


def assemble(blocks, mats, cplx):
    """the matrix with mats[b] on blocks[b] and exact zeros elsewhere"""
    a = np.zeros((sum(len(r) for r, _ in blocks), sum(len(c) for _, c in blocks)), dtype=complex if cplx else float)
    for (rows, cols), x in zip(blocks, mats):
        a[np.ix_(rows, cols)] = x
    return a


def adjoint(a, blocks):
    """the same call for system R: the adjoint matrix, every block's index lists swapped"""
    return np.ascontiguousarray(a.conj().T), [(c, r) for r, c in blocks]


def offsets(blocks):
    """(row index list, row offsets, column index list, column offsets) as mpse_block_qr takes them"""
    rows = np.concatenate([b[0] for b in blocks]).astype(np.int64)
    cols = np.concatenate([b[1] for b in blocks]).astype(np.int64)
    roff = np.cumsum([0] + [len(b[0]) for b in blocks]).astype(np.int64)
    coff = np.cumsum([0] + [len(b[1]) for b in blocks]).astype(np.int64)
    return rows, roff, cols, coff


def single_cases(n):
    """[(class, m)] of the one-block calls of width n"""
    return [(cls, m) for m in heights(n) for cls in classes_of(n)]


def single(cls, m, n, cplx):
    """(a, blocks, widths, classes) of a one-block call: the block itself, rows and columns in order"""
    return block(cls, m, n, cplx), [(np.arange(m, dtype=np.int64), np.arange(n, dtype=np.int64))], [n], [cls]


# six ragged blocks whose decisions differ, one call through the left-looking kernel (161 columns); without that block
# the same call goes through the right-looking one
MIXED = ((40, 17, "I"), (33, 33, "II"), (100, 48, "III"), (300, 161, "IV"), (64, 16, "II"), (20, 1, "I"))
MIXED_ZERO_COLUMN = (1, 5)      # (block, column) zeroed for the fallback case: inside the 33 x 33 block


def mixed(cplx, wide=True, zero_column=False):
    """(a, blocks, widths, classes) of the MIXED call; ``wide`` False leaves the 161-column block out, ``zero_column``
    zeroes one column of the 33 x 33 block (pass 2 has nothing to normalise there: the device flag goes up)"""
    spec = [s for s in MIXED if wide or s[1] <= RL_MAX_COLS]
    mats = [block(c, m, n, cplx) for m, n, c in spec]
    if zero_column:
        b, j = MIXED_ZERO_COLUMN
        assert spec[b][:2] == (33, 33)
        mats[b][:, j] = 0
    blocks = layout([(m, n) for m, n, _ in spec], seed=len(spec))
    return assemble(blocks, mats, cplx), blocks, [n for _, n, _ in spec], [c for _, _, c in spec]
