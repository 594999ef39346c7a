"""mpse_block_svd / mpse_block_svd_full on BOTH sweep kernels, each at the widths it was written for, against the
constructed singular systems of tests/svd_problems.py (values known by construction; LAPACK meets the same checks at
1e-13 on the same matrices: tests/test_svd_problems_host.py).

Which kernel ran is asserted from mpse_block_svd_stats, and every width is sized from the dynamic LDS the column
kernel was granted in this process (entry 6 of the counters: T = lds / 512 complex, lds / 256 real columns), so a
threshold that moves - or a runtime that grants 64 KB instead of 150 - cannot take a case off its path silently.

Bounds: the project's contract for the decomposition (test_engine_gpu.py, and what the sweeps above this layer rely
on) - values, per block, and reconstruction to 1e-13 while the widest block has fewer than 250 columns, 1e-12 above;
both factors isometries to 1e-12; exact zeros outside a block's rows and columns.  Every case prints its figures
(path counters, gram_R, sweeps, worst deviations) before it asserts: run with ``-s``.

Measured on the MI355X with the 150 KB grant (LAPACK on the same matrices: values 3e-15, reconstruction 4e-15,
orthogonality 4e-15), worst over the graded and the stepped spectrum:
  Gram kernel, 304 / 313 complex columns: values 4.1e-14, reconstruction 6.2e-14, orthogonality 1.3e-13 (11 - 19 sweeps)
  Gram kernel, 604 / 613 real columns:    values 1.2e-13, reconstruction 3.2e-13, orthogonality 3.3e-13 (12 - 17 sweeps)
  column kernel, 300 complex / 600 real:  values 1.0e-13, reconstruction 3.0e-13, orthogonality 4.9e-13
  every case below 250 columns:           values 1.7e-14, reconstruction 1.8e-14, orthogonality 7.8e-14"""
import ctypes as C

import numpy as np
import pytest

from renormalizer_amd import engine as E
import svd_problems as sp            # (tests/svd_problems.py)

pytestmark = pytest.mark.gpu

COUNTS = ("decompositions", "column", "gram", "sweeps", "launches")


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


@pytest.fixture(scope="module")
def lds(eng):
    """bytes of dynamic LDS of the column kernel: known after the first decomposition of the process"""
    a, blocks, _ = sp.tiny_blocks(1)
    dev_block_svd_full(eng, a, blocks)
    v = eng.block_svd_stats()["column_lds"]
    assert v in (150 * 1024, 64 * 1024)
    return v


@pytest.fixture(scope="module")
def problems(lds):
    """the matrices of sp.cases(lds), built once and left unchanged: name -> (a, blocks, s_blocks)"""
    cases, built = sp.cases(lds), {}

    def get(name):
        if name not in built:
            built[name] = sp.build_case(cases[name])
            built[name][0].setflags(write=False)
        return built[name]
    return get


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    monkeypatch.delenv("MPSE_SVD_GRAM", raising=False)
    monkeypatch.delenv("MPSE_SVD_GRAM_R", raising=False)


def dev_block_svd_full(eng, a, blocks, extra=None, check=True):
    """(u, s, vt) of ``mpse_block_svd`` (extra None) or ``mpse_block_svd_full`` called directly: u (nrow x KU),
    vt (KV x ncol) with the extra null vectors of the taller side of block b after column / row K.  ``check`` False:
    the status instead of an exception."""
    rows, roff, cols, coff = sp.offsets(blocks)
    nrow, ncol = a.shape
    K = int(sum(min(len(ls), len(rs)) for ls, rs in blocks))
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_int64))
    A = eng.asdevice(np.ascontiguousarray(a))
    S = np.zeros(K)
    sp_ = S.ctypes.data_as(C.POINTER(C.c_double))
    if extra is None:
        U, Vt = eng.empty((nrow, K), a.dtype), eng.empty((K, ncol), a.dtype)
        st = eng.lib.mpse_block_svd(eng.ctx, A.code, A.ptr, nrow, ncol, len(blocks), p(rows), p(roff), p(cols), p(coff),
                                    U.ptr, Vt.ptr, sp_, K)
    else:
        ex = np.asarray(extra, dtype=np.int64)
        tall = np.array([len(ls) >= len(rs) for ls, rs in blocks])
        KU, KV = K + int(np.clip(ex, 0, None)[tall].sum()), K + int(np.clip(ex, 0, None)[~tall].sum())
        U, Vt = eng.empty((nrow, KU), a.dtype), eng.empty((KV, ncol), a.dtype)
        st = eng.lib.mpse_block_svd_full(eng.ctx, A.code, A.ptr, nrow, ncol, len(blocks), p(rows), p(roff), p(cols),
                                         p(coff), p(ex), U.ptr, KU, Vt.ptr, KV, sp_, K)
    if not check:
        return st
    eng._check(st)
    return U.to_host(), S, Vt.to_host()


def run(eng, a, blocks, path, extra=None):
    """One decomposition that must run its sweeps in ``path`` ("column" / "gram"): (u, s, vt, counters of the call)"""
    s0 = eng.block_svd_stats()
    u, s, vt = dev_block_svd_full(eng, a, blocks, extra)
    s1 = eng.block_svd_stats()
    d = {k: s1[k] - s0[k] for k in COUNTS}
    d["gram_R"] = s1["gram_R"]
    assert s1["column_lds"] == s0["column_lds"]
    assert (d["decompositions"], d[path], d["column"] + d["gram"]) == (1, 1, 1), (path, d)
    assert d["sweeps"] >= 1 and d["launches"] >= d["sweeps"], d
    return u, s, vt, d


def tol_of(blocks):
    return sp.contract_tol([min(len(ls), len(rs)) for ls, rs in blocks])


def checked(eng, name, prob, path, label=""):
    """run + the contract, figures printed first"""
    a, blocks, s_blocks = prob
    u, s, vt, d = run(eng, a, blocks, path)
    tol, tol_o = tol_of(blocks)
    rep = lambda f: print(f"\n[block_svd] {name}{label} path={path} gram_R={d['gram_R'] if path == 'gram' else '-'} "
                          f"sweeps={d['sweeps']} launches={d['launches']} values={f['values']:.2e} recon={f['recon']:.2e} "
                          f"orth_u={f['orth_u']:.2e} orth_vt={f['orth_vt']:.2e} (tol {tol:g})")
    sp.check_svd(a, blocks, u, s, vt, s_blocks, tol, tol_o, report=rep)
    return u, s, vt, d


def gram_r_rule(nn, nblk=1):
    """row slabs per pair of column blocks for a widest block of nn columns: a 16-row tile of [X; V] per wave, halved
    while slabs x pairs x blocks exceed 1024 workgroups per launch, at most 16"""
    nb = -(-nn // 16)
    r, pairs = (2 * nb + 3) // 4, ((nb + 1) & ~1) // 2
    while r > 1 and r * pairs * nblk > 1024:
        r //= 2
    return min(r, 16)


def tname(cplx):
    return "c128" if cplx else "f64"


@pytest.mark.parametrize("spec", ["graded", "steps"])
@pytest.mark.parametrize("over", [4, 13])
@pytest.mark.parametrize("cplx", [True, False])
def test_natural_gram_path_one_block(eng, lds, problems, cplx, over, spec):
    """Widths T + 4 and T + 13 (a multiple of neither 4 nor 16: the row clamp of the Gram loads and a partial last
    column block), no switch set: the Gram kernel, with the gram_R its rule gives"""
    T = sp.widest(lds)[0 if cplx else 1]
    name = f"gram+{over}-{spec}-{tname(cplx)}"
    _, _, _, d = checked(eng, name, problems(name), "gram")
    assert d["gram_R"] == gram_r_rule(T + over)


@pytest.mark.parametrize("spec", ["graded", "steps"])
@pytest.mark.parametrize("cplx,which", [(True, "top"), (False, "top"), (True, "pass2-257")])
def test_same_matrix_through_both_kernels(eng, lds, problems, monkeypatch, cplx, which, spec):
    """Width T exactly - the widest block of the column kernel - and, complex, 257 columns (the smallest width that
    takes the second pass of the Gram row loop): the column kernel (where the block fits), then the same matrix under
    MPSE_SVD_GRAM=2.  Both meet the contract; their values agree within 2 tol s_max (each is within tol of the
    constructed ones)."""
    T =sp.widest(lds)[0 if cplx else 1]
    name = f"{which}-{spec}-{tname(cplx)}"
    prob = problems(name)
    n = prob[0].shape[1]
    assert n == (T if which == "top" else 257)
    _, s_nat, _, _ = checked(eng, name, prob, "column" if n <= T else "gram")
    monkeypatch.setenv("MPSE_SVD_GRAM", "2")
    _, s_gram, _, d = checked(eng, name, prob, "gram", " forced")
    assert d["gram_R"] == gram_r_rule(n)
    tol, _ = tol_of(prob[1])
    smax = max(x.max() for x in prob[2])
    print(f"[block_svd] {name} column vs Gram values: {np.abs(s_nat - s_gram).max() / smax:.2e}")
    assert np.abs(s_nat - s_gram).max() <= 2 * tol * smax


@pytest.mark.parametrize("spec", ["graded", "steps"])
@pytest.mark.parametrize("cplx", [True, False])
def test_row_slabs_bitwise(eng, problems, monkeypatch, cplx, spec):
    """Forced Gram, one block of 72 columns (10 row tiles of [X; V]; default R = 3, an uneven deal): every slab count
    returns the same bits - the slabs repeat the Gram matrix and the rotations on the same inputs and the row update
    is row-independent - and the counter reports the R that ran"""
    name = f"slabs72-{spec}-{tname(cplx)}"
    prob = problems(name)
    monkeypatch.setenv("MPSE_SVD_GRAM", "2")
    u0, s0, vt0, d0 = checked(eng, name, prob, "gram", " default R")
    assert d0["gram_R"] == 3 == gram_r_rule(72)
    for R in (1, 3, 7, 16):
        monkeypatch.setenv("MPSE_SVD_GRAM_R", str(R))
        u, s, vt, d = run(eng, prob[0], prob[1], "gram")
        assert d["gram_R"] == R
        assert (d["sweeps"], d["launches"]) == (d0["sweeps"], d0["launches"])
        assert np.array_equal(s, s0) and np.array_equal(u, u0) and np.array_equal(vt, vt0), R


@pytest.mark.parametrize("last", ["graded", "zero"])
@pytest.mark.parametrize("cplx", [True, False])
def test_ragged_blocks_on_the_gram_path(eng, lds, problems, cplx, last):
    """Five blocks in one call whose widest, T + 4 columns, puts all of them on the Gram path: (T+13) x (T+4) graded,
    150 x 70 steps, 17 x 40 flat (wide: factorised as its adjoint; nothing to rotate), 9 x 1, 33 x 33 graded or all
    zero.  They converge in different sweeps while every launch copies X and V of all of them between the two buffers."""
    T = sp.widest(lds)[0 if cplx else 1]
    name = f"ragged-{last}-{tname(cplx)}"
    prob = problems(name)
    assert [(len(ls), len(rs)) for ls, rs in prob[1]] == [(T + 13, T + 4), (150, 70), (17, 40), (9, 1), (33, 33)]
    _, _, _, d = checked(eng, name, prob, "gram")
    assert d["gram_R"] == gram_r_rule(T + 4, 5)


@pytest.mark.parametrize("spec", ["graded", "steps"])
@pytest.mark.parametrize("cplx", [True, False])
def test_many_blocks_and_the_slab_clamp(eng, problems, monkeypatch, cplx, spec):
    """120 blocks - 90 x 72 and 119 of up to 6 x 6: forced onto the Gram kernel, 3 slabs x 3 pairs x 120 blocks exceed
    1024 workgroups per launch and R drops from 3 to 1; without the switch the column kernel takes the call"""
    name = f"many-{spec}-{tname(cplx)}"
    prob = problems(name)
    assert len(prob[1]) == 120
    checked(eng, name, prob, "column")
    monkeypatch.setenv("MPSE_SVD_GRAM", "2")
    _, _, _, d = checked(eng, name, prob, "gram", " forced")
    assert d["gram_R"] == 1


@pytest.mark.parametrize("nblk", [2000, 2001])
def test_read_back_boundary(eng, nblk):
    """2000 blocks: the done words of a sweep come back through the published slot; 2001: through a copy.  Real 2 x 2
    blocks with distinct values, column kernel."""
    checked(eng, f"tiny-{nblk}-f64", sp.tiny_blocks(nblk), "column")


@pytest.mark.parametrize("path", ["column", "gram"])
@pytest.mark.parametrize("cplx", [True, False])
def test_full_extras_on_both_sides(eng, problems, monkeypatch, cplx, path):
    """mpse_block_svd_full with null vectors asked for on both sides in one call: blocks (m, n, extra) = (40, 12, 28),
    (40, 12, 5), (12, 40, 12), (9, 9, 0), (1, 6, 5), (30, 30, 0)"""
    name = f"full-{tname(cplx)}"
    a, blocks, s_blocks = problems(name)
    extra = [b[2] for b in sp.FULL_BLOCKS]
    assert [(len(ls), len(rs)) for ls, rs in blocks] == [b[:2] for b in sp.FULL_BLOCKS]
    if path == "gram":
        monkeypatch.setenv("MPSE_SVD_GRAM", "2")
    u, s, vt, d = run(eng, a, blocks, path, extra)
    K = len(s)
    assert K == 76 and u.shape == (a.shape[0], K + 33) and vt.shape == (K + 17, a.shape[1])
    tol, tol_o = tol_of(blocks)
    rep = lambda f: print(f"\n[block_svd] {name} full path={path} sweeps={d['sweeps']} values={f['values']:.2e} "
                          f"recon={f['recon']:.2e} orth_u={f['orth_u']:.2e} orth_vt={f['orth_vt']:.2e} (tol {tol:g})")
    sp.check_svd(a, blocks, u[:, :K], s, vt[:K], s_blocks, tol, tol_o, report=rep)
    mu, mvt = np.zeros(u.shape, dtype=bool), np.zeros(vt.shape, dtype=bool)       # where extras may stand
    ko, uo, vo, worst_o, worst_n = 0, K, K, 0.0, 0.0
    for (ls, rs), sb, ex in zip(blocks, s_blocks, extra):
        m, n = len(ls), len(rs)
        k = min(m, n)
        ab = a[np.ix_(ls, rs)]
        if m >= n:        # extras: columns of U after K, in block order; orthonormal with the economic ones, A_b^H x = 0
            x = u[ls, uo:uo + ex]
            mu[ls, uo:uo + ex] = True
            side = np.concatenate([u[ls, ko:ko + k], x], axis=1)
            null = np.abs(ab.conj().T @ x).max() if ex else 0.0
            uo += ex
        else:             # rows of Vt after K: A_b y^H = 0
            y = vt[vo:vo + ex][:, rs]
            mvt[vo:vo + ex, rs] = True
            side = np.concatenate([vt[ko:ko + k][:, rs], y], axis=0).conj().T
            null = np.abs(ab @ y.conj().T).max() if ex else 0.0
            vo += ex
        assert side.shape[1] == k + ex
        worst_o = max(worst_o, float(np.abs(side.conj().T @ side - np.eye(k + ex)).max()))
        worst_n = max(worst_n, float(null) / sb.max())
        ko += k
    print(f"[block_svd] {name} full path={path} extras: orthonormality {worst_o:.2e}, |A^H x| / s_max {worst_n:.2e}")
    assert (uo, vo) == (u.shape[1], vt.shape[0])
    assert worst_o <= tol_o and worst_n <= tol
    # exactly zero outside the block, and the shorter side of a block receives nothing
    assert not np.any(u[:, K:][~mu[:, K:]]) and not np.any(vt[K:][~mvt[K:]])


def test_full_refuses_bad_extra_counts(eng, problems):
    """more null vectors than the taller side has (29 of 40 - 12), and a negative count: MPSE_ERR_SHAPE before any
    device work, counters unchanged"""
    a, blocks, _ = problems("full-f64")
    extra = [b[2] for b in sp.FULL_BLOCKS]
    s0 = eng.block_svd_stats()
    for bad in ([29] + extra[1:], extra[:1] + [-1] + extra[2:]):
        assert dev_block_svd_full(eng, a, blocks, bad, check=False) == E.MPSE_ERR_SHAPE
    assert eng.block_svd_stats() == s0
