"""The Cholesky-QR kernels of mpse_block_qr (mpse_cholqr.hip) on every pass decision, both factor kernels and every tile
edge, on the constructed blocks of tests/qr_problems.py.  What each block makes the device decide - two or three passes,
first-order or plain last factor - is predicted by the float64 emulation of the device rule in that module with a
margin of 100 to both thresholds (tests/test_qr_problems_host.py) and asserted here from mpse_block_qr_path_stats,
together with which factor kernel took the call.

Every decomposition is held to the project's contract for the block QR (test_engine_gpu.py): relerr(U Vt, A) < 1e-13,
max|iso^H iso - I| < 1e-13, the other factor of every block exactly triangular; on top of it the diagonal of a
Cholesky-QR factor is real and positive, and U and Vt - filled with NaN on the device before the call - come back
exactly zero outside the blocks and without a NaN inside.  Both dtypes, both systems (system R: the adjoint layout).

Heights (qr_problems.heights; 32 rows per chunk for every block here on a device of 256 compute units): the square
block and the one of one or two rows more give ceil(m / 32) row chunks with the last one partly filled - 1 chunk up to
31 rows, 1 / 2 at 32 columns, 2 at 33 (33 x 33: one row in the second), 5 at 145, 5 / 6 at 160, 6 at 161 and 176, 8 / 9
at 255 and 256 (257 rows: one row in the ninth) - and the third height 5 (130, 150, 155 rows), 6 (170, 185, 190) or
7 (200, 203, 210, 220) chunks, i.e. two macro chunks of four waves with 1, 2 or 3 waves in the second; 650 and 700 rows
under 255 and 256 columns, which cannot have fewer than 8 chunks: 21 and 22, six macro chunks.  No height is a multiple of 16 except the square 16, 32, 160, 176 and 256: the last workgroup of k_cq_trsm is
ragged everywhere else.

Every case prints its counters before it asserts: run with ``-s``."""
import ctypes as C

import numpy as np
import pytest

from renormalizer_amd import engine as E
import qr_problems as qp            # (tests/qr_problems.py)

pytestmark = pytest.mark.gpu

TOL = 1e-13


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


@pytest.fixture(scope="module")
def mixed_problems():
    """(cplx, wide, zero_column) -> the mixed call of qr_problems.mixed, built once and left unchanged"""
    built = {}

    def get(cplx, wide=True, zero_column=False):
        key = (cplx, wide, zero_column)
        if key not in built:
            built[key] = qp.mixed(cplx, wide=wide, zero_column=zero_column)
            built[key][0].setflags(write=False)
        return built[key]
    return get


def _relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(b).max()))


def dev_block_qr(eng, a, blocks, system, flags=0):
    """(u, vt) of ``mpse_block_qr`` called directly on the blocks [(rows, cols)]; U and Vt hold NaN before the call"""
    rows, roff, cols, coff = qp.offsets(blocks)
    nrow, ncol = a.shape
    K = int(sum(min(len(r), len(c)) for r, c in blocks))
    nan = np.nan * (1 + 1j) if np.iscomplexobj(a) else np.nan
    A = eng.asdevice(np.ascontiguousarray(a))
    U, Vt = eng.asdevice(np.full((nrow, K), nan, dtype=a.dtype)), eng.asdevice(np.full((K, ncol), nan, dtype=a.dtype))
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_int64))
    eng._check(eng.lib.mpse_block_qr(eng.ctx, A.code, A.ptr, nrow, ncol, len(blocks), p(rows), p(roff), p(cols), p(coff),
                                     int(system == "R") | flags, U.ptr, Vt.ptr, K))
    return U.to_host(), Vt.to_host()


def check_contract(a, blocks, u, vt, system, tag, positive_diagonal=True):
    """the contract of the block QR for one decomposition; returns (reconstruction, orthogonality)"""
    assert not np.any(np.isnan(u)) and not np.any(np.isnan(vt)), (tag, "NaN left in U / Vt")
    mu, mv = np.ones(u.shape, dtype=bool), np.ones(vt.shape, dtype=bool)
    k0 = 0
    for b, (rows, cols) in enumerate(blocks):
        k = min(len(rows), len(cols))
        mu[np.ix_(rows, np.arange(k0, k0 + k))] = False
        mv[np.ix_(np.arange(k0, k0 + k), cols)] = False
        # the triangular factor of the block: R (upper) in Vt for system L, L = R^H (lower) in U for system R
        tri = vt[k0:k0 + k][:, cols] if system == "L" else u[rows][:, k0:k0 + k].conj().T
        assert np.abs(np.tril(tri, -1)).max(initial=0.0) == 0, (tag, b, "factor not triangular")
        if positive_diagonal:
            d = np.diagonal(tri)
            assert np.all(d.imag == 0) and np.all(d.real > 0), (tag, b, "diagonal of the factor", d)
        k0 += k
    assert not np.any(u[mu]) and not np.any(vt[mv]), (tag, "nonzero outside the blocks")
    rec = _relerr(u @ vt, a)
    iso = u if system == "L" else vt.conj().T
    orth = float(np.abs(iso.conj().T @ iso - np.eye(iso.shape[1])).max())
    assert rec < TOL, (tag, "reconstruction", rec)
    assert orth < TOL, (tag, "orthogonality", orth)
    return rec, orth


def run_call(eng, a, blocks, expect, tag, positive_diagonal=True):
    """The call in both systems, each held to the contract and to the counters ``expect``; [(u, vt)] per system"""
    out = []
    for system in ("L", "R"):
        x, xb = (a, blocks) if system == "L" else qp.adjoint(a, blocks)
        s0 = eng.block_qr_path_stats()
        u, vt = dev_block_qr(eng, x, xb, system)
        d = eng.block_qr_path_stats(since=s0)
        print(f"\n[block_qr] {tag} system {system}: {tuple(d.values())}", end="")
        rec, orth = check_contract(x, xb, u, vt, system, (tag, system), positive_diagonal)
        print(f" recon {rec:.1e} orth {orth:.1e}", end="")
        assert d == expect, (tag, system, "path counters", d, "predicted", expect)
        out.append((u, vt))
    return out


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("n", qp.WIDTHS)
def test_single_block_edges(eng, n, cplx):
    """One block of n columns at its three heights, in every decision class that exists for the width: the counters of
    each call are those of its class and of the factor kernel of its width (right-looking up to 160 columns)"""
    try:
        eng.block_qr_scheme(2)
        for cls, m in qp.single_cases(n):
            a, blocks, ws, cs = qp.single(cls, m, n, cplx)
            run_call(eng, a, blocks, qp.predict(ws, cs), f"{m} x {n} class {cls} {'c128' if cplx else 'f64'}")
    finally:
        eng.block_qr_scheme(-1)


@pytest.mark.parametrize("cplx", [True, False])
def test_257_columns_take_householder(eng, cplx):
    """one column more than the Cholesky-QR kernels take: no counter of the path moves, the contract holds"""
    try:
        eng.block_qr_scheme(2)
        a, blocks, _, _ = qp.single("II", 300, 257, cplx)
        run_call(eng, a, blocks, qp.NO_CHANGE, f"300 x 257 {'c128' if cplx else 'f64'}", positive_diagonal=False)
    finally:
        eng.block_qr_scheme(-1)


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("cplx", [True, False])
def test_mixed_blocks_one_call(eng, mixed_problems, cplx, wide):
    """Six ragged blocks of all four classes in ONE call, rows and columns interleaved: the 161-column block takes the
    whole call - the 1-, 16- and 17-column blocks with it - through the left-looking kernel (blocks, two-pass,
    first-order at pass 2, at pass 3: 6, 4, 2, 1); without it the same call goes through the right-looking one
    (5, 4, 2, 1).  Twice each: bitwise the same U and Vt."""
    a, blocks, ws, cs = mixed_problems(cplx, wide)
    expect = qp.predict(ws, cs)
    assert tuple(expect.values()) == ((1, 0, 1, 0, 6, 4, 2, 1) if wide else (1, 1, 0, 0, 5, 4, 2, 1))
    tag = f"mixed {'six' if wide else 'five'} blocks {'c128' if cplx else 'f64'}"
    try:
        eng.block_qr_scheme(2)
        first = run_call(eng, a, blocks, expect, tag)
        again = run_call(eng, a, blocks, expect, tag + " (repeat)")
    finally:
        eng.block_qr_scheme(-1)
    for (u0, v0), (u1, v1), system in zip(first, again, "LR"):
        assert np.array_equal(u0, u1) and np.array_equal(v0, v1), (tag, system, "not bitwise repeatable")


@pytest.mark.parametrize("cplx", [True, False])
def test_fallback_inside_mixed_call(eng, mixed_problems, cplx):
    """The six-block call with one exactly zero column in the 33 x 33 block: the Cholesky-QR kernels are tried (left-
    looking: the 161-column block), pass 2 finds nothing to normalise, the flag goes up and the Householder kernels redo
    the whole call - every block still meets the contract (the Householder factor's diagonal has no sign convention)."""
    a, blocks, ws, _ = mixed_problems(cplx, True, True)
    try:
        eng.block_qr_scheme(2)
        for system in ("L", "R"):
            x, xb = (a, blocks) if system == "L" else qp.adjoint(a, blocks)
            s0 = eng.block_qr_path_stats()
            u, vt = dev_block_qr(eng, x, xb, system)
            d = eng.block_qr_path_stats(since=s0)
            tag = ("zero column", "c128" if cplx else "f64", system)
            print(f"\n[block_qr] {tag}: {tuple(d.values())}", end="")
            assert (d["chol_calls"], d["right_looking"], d["left_looking"], d["fallbacks"]) == (1, 0, 1, 1), (tag, d)
            assert d["blocks"] == len(ws), (tag, d)          # the scatter of the refused attempt counted its blocks
            check_contract(x, xb, u, vt, system, tag, positive_diagonal=False)
            assert eng.block_qr_check() is False, tag         # optimistic mode off: verified as it ran, nothing pending
    finally:
        eng.block_qr_scheme(-1)


def test_pass_stats_agree_with_path_stats(eng, mixed_problems):
    """mpse_block_qr_pass_stats: NULL for either pointer, the values of entries 4 and 5 of mpse_block_qr_path_stats
    before and after a Cholesky-QR call, and no counter moved by a Householder-only decomposition (scheme 0, and bit 1
    of system_is_R under scheme 2); entries past the last one come back zero."""
    a, blocks, ws, cs = mixed_problems(True, False)

    def both():
        x, y = C.c_int64(-1), C.c_int64(-1)
        eng._check(eng.lib.mpse_block_qr_pass_stats(eng.ctx, C.byref(x), None))
        eng._check(eng.lib.mpse_block_qr_pass_stats(eng.ctx, None, C.byref(y)))
        eng._check(eng.lib.mpse_block_qr_pass_stats(eng.ctx, None, None))
        assert (x.value, y.value) == eng.block_qr_pass_stats()
        s = eng.block_qr_path_stats()
        assert (x.value, y.value) == (s["blocks"], s["two_pass"]), (x.value, y.value, s)
        st = eng.block_qr_stats()
        assert (st[1], st[2]) == (s["chol_calls"], s["fallbacks"]) and s["chol_calls"] == s["right_looking"] + s["left_looking"]
        return s

    try:
        eng.block_qr_scheme(2)
        s0 = both()
        dev_block_qr(eng, a, blocks, "L")
        s1 = both()
        assert {k: s1[k] - s0[k] for k in s0} == qp.predict(ws, cs)
        u, vt = dev_block_qr(eng, a, blocks, "L", flags=2)            # this decomposition by Householder
        assert both() == s1
        check_contract(a, blocks, u, vt, "L", "bit 1 of system_is_R", positive_diagonal=False)
        eng.block_qr_scheme(0)
        u, vt = dev_block_qr(eng, a, blocks, "L")
        assert both() == s1
        check_contract(a, blocks, u, vt, "L", "scheme 0", positive_diagonal=False)
    finally:
        eng.block_qr_scheme(-1)
    v = (C.c_int64 * 12)(*([-7] * 12))
    eng._check(eng.lib.mpse_block_qr_path_stats(eng.ctx, v, 12))
    assert list(v[:8]) == list(s1.values()) and list(v[8:]) == [0] * 4
    v = (C.c_int64 * 3)(-7, -7, -7)
    eng._check(eng.lib.mpse_block_qr_path_stats(eng.ctx, v, 2))
    assert list(v) == [s1["chol_calls"], s1["right_looking"], -7]
    eng._check(eng.lib.mpse_block_qr_path_stats(eng.ctx, None, 0))
    assert eng.lib.mpse_block_qr_path_stats(eng.ctx, None, 3) != 0 and eng.lib.mpse_block_qr_path_stats(eng.ctx, v, -1) != 0


def test_optimistic_mode_clears_only_the_breakdown_word(eng, mixed_problems):
    """switching the optimistic mode on and off clears the sticky word and leaves every counter as it was"""
    a, blocks, _, _ = mixed_problems(False, False)
    try:
        eng.block_qr_scheme(2)
        dev_block_qr(eng, a, blocks, "L")
        s0 = eng.block_qr_path_stats()
        assert s0["blocks"] >= 5 and s0["first_order_pass2"] >= 2 and s0["first_order_pass3"] >= 1
        eng.block_qr_optimistic(True)
        assert eng.block_qr_path_stats() == s0 and eng.block_qr_check() is False
        eng.block_qr_optimistic(False)
        assert eng.block_qr_path_stats() == s0
    finally:
        eng.block_qr_optimistic(False)
        eng.block_qr_scheme(-1)
