"""Quantum-number blocked matrices with exactly known singular systems, shared by the host and GPU tests of the block SVD.

Every block is U diag(s) V^H with U, V from ``np.linalg.qr`` of Gaussian matrices and a spectrum chosen by name, placed
on its own quantum-number sector with rows and columns permuted, so the singular values a decomposition must return
are the constructed ones - no second decomposition stands between the kernel and its reference.  ``check_svd`` is the
one statement of what a block SVD owes its callers; ``cases`` lists the layouts of tests/test_block_svd_gpu.py, sized
from the widest block the column kernel takes, so that the host test proves LAPACK meets the same bounds on the same
matrices."""
import numpy as np


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return a


def spectrum(name, k):
    """The k singular values (descending) of a named spectrum; anything but a name is taken as the values themselves.
      graded  exp(-30 i / k), the last 5 exactly zero when k > 10
      steps   clusters of 8 equal values 2^-j, the last 5 exactly zero when k > 10 (degenerate: the vectors are not
              unique, every property check_svd asserts is)
      flat    all ones: the block has orthonormal columns (rows), a first sweep finds nothing to rotate
      zero    an all-zero block"""
    if not isinstance(name, str):
        s = np.sort(np.atleast_1d(np.asarray(name, dtype=float)))[::-1]
        assert s.shape == (k,) and np.all(s >= 0)
        return s
    i = np.arange(k)
    if name == "graded":
        s = np.exp(-30.0 * i / k)
    elif name == "steps":
        s = 2.0 ** -(i // 8).astype(float)
    elif name == "flat":
        return np.ones(k)
    elif name == "zero":
        return np.zeros(k)
    else:
        raise ValueError(name)
    if k > 10:
        s[-5:] = 0.0
    return s


def block_matrix(rng, heights, widths, spectra, cplx, permute=True):
    """(a, qnl, qnr, s_blocks): block b of ``a`` is U_b diag(s_b) V_b^H (heights[b] x widths[b]) on the rows of charge b
    and the columns of charge -b (total charge 0), zero elsewhere; ``s_blocks[b]`` are its min(h, w) constructed values."""
    heights, widths = list(heights), list(widths)
    assert len(heights) == len(widths) == len(spectra)
    m, n = sum(heights), sum(widths)
    a = np.zeros((m, n), dtype=complex if cplx else float)
    qnl = np.repeat(np.arange(len(heights)), heights)
    qnr = -np.repeat(np.arange(len(widths)), widths)
    if permute:
        qnl, qnr = rng.permutation(qnl), rng.permutation(qnr)
    s_blocks = []
    for (ls, rs), h, w, sp in zip(sector_blocks(qnl, qnr), heights, widths, spectra):
        k = min(h, w)
        s = spectrum(sp, k)
        if np.any(s != 0):
            u, _ = np.linalg.qr(_rand(rng, (h, k), cplx))
            v, _ = np.linalg.qr(_rand(rng, (w, k), cplx))
            a[np.ix_(ls, rs)] = (u * s) @ v.conj().T
        s_blocks.append(s)
    return a, qnl[:, None], qnr[:, None], s_blocks


def sector_blocks(qnl, qnr):
    """[(rows, cols)] of the sectors of total charge 0 in ascending order of the left charge (the order of
    ``qn_blocks``), index lists ascending."""
    ql, qr = np.asarray(qnl).reshape(-1), -np.asarray(qnr).reshape(-1)
    ol, orr = np.argsort(ql, kind="stable"), np.argsort(qr, kind="stable")
    vl, sl = np.unique(ql[ol], return_index=True)
    vr, sr = np.unique(qr[orr], return_index=True)
    assert np.array_equal(vl, vr)
    return list(zip(np.split(ol, sl[1:]), np.split(orr, sr[1:])))


def offsets(blocks):
    """(row index list, row offsets, column index list, column offsets) as the engine's entry points take them"""
    rows = np.concatenate([b[0] for b in blocks]).astype(np.int64)
    cols = np.concatenate([b[1] for b in blocks]).astype(np.int64)
    roff = np.cumsum([0] + [len(b[0]) for b in blocks]).astype(np.int64)
    coff = np.cumsum([0] + [len(b[1]) for b in blocks]).astype(np.int64)
    return rows, roff, cols, coff


def lapack_svd(a, blocks):
    """(u, s, vt) of the blocked matrix by ``np.linalg.svd`` block by block, in the engine's layout"""
    K = sum(min(len(ls), len(rs)) for ls, rs in blocks)
    u, vt, s = np.zeros((a.shape[0], K), dtype=a.dtype), np.zeros((K, a.shape[1]), dtype=a.dtype), np.zeros(K)
    ko = 0
    for ls, rs in blocks:
        k = min(len(ls), len(rs))
        bu, bs, bvt = np.linalg.svd(a[np.ix_(ls, rs)], full_matrices=False)
        u[ls, ko:ko + k], s[ko:ko + k], vt[ko:ko + k, rs] = bu, bs, bvt
        ko += k
    return u, s, vt


def svd_figures(a, blocks, u, s, vt, s_blocks):
    """What check_svd measures: {"values": max_b max|s - s_b| / max(s_b) (blocks with max(s_b) = 0 must return zeros
    and count under "zero_block_values" with their largest value), "recon": |(u s) vt - a|_F / |a|_F, "orth_u",
    "orth_vt": max|u^H u - 1|, max|vt vt^H - 1|, "descending", "outside": entries of u / vt outside their blocks}.
    u and vt vanish outside their blocks' rows / columns exactly (asserted here), so the products are formed block by
    block: the same numbers as from the dense products, without their cost for thousands of blocks."""
    K = s.shape[0]
    assert u.shape == (a.shape[0], K) and vt.shape == (K, a.shape[1])
    mu, mvt, ma = np.zeros(u.shape, dtype=bool), np.zeros(vt.shape, dtype=bool), np.zeros(a.shape, dtype=bool)
    ko = 0
    for ls, rs in blocks:
        k = min(len(ls), len(rs))
        mu[ls, ko:ko + k] = True
        mvt[ko:ko + k, rs] = True
        ma[np.ix_(ls, rs)] = True
        ko += k
    assert ko == K
    assert not np.any(a[~ma]), "the input has entries outside its blocks"
    fig = {"outside": int(np.count_nonzero(u[~mu]) + np.count_nonzero(vt[~mvt])), "values": 0.0,
           "zero_block_values": 0.0, "orth_u": 0.0, "orth_vt": 0.0, "descending": True}
    err2, ko = 0.0, 0
    for (ls, rs), sb in zip(blocks, s_blocks):
        k = min(len(ls), len(rs))
        bu, bs, bvt, ab = u[ls, ko:ko + k], s[ko:ko + k], vt[ko:ko + k][:, rs], a[np.ix_(ls, rs)]
        assert sb.shape == (k,)
        if sb.max() > 0:
            fig["values"] = max(fig["values"], float(np.abs(bs - sb).max() / sb.max()))
        else:
            fig["zero_block_values"] = max(fig["zero_block_values"], float(np.abs(bs).max()))
        fig["descending"] = fig["descending"] and bool(np.all(np.diff(bs) <= 0))
        err2 += float(np.linalg.norm((bu * bs) @ bvt - ab) ** 2)
        fig["orth_u"] = max(fig["orth_u"], float(np.abs(bu.conj().T @ bu - np.eye(k)).max()))
        fig["orth_vt"] = max(fig["orth_vt"], float(np.abs(bvt @ bvt.conj().T - np.eye(k)).max()))
        ko += k
    na = float(np.linalg.norm(a))
    fig["recon"] = float(np.sqrt(err2)) / na if na > 0 else float(np.sqrt(err2))
    return fig


def check_svd(a, blocks, u, s, vt, s_blocks, tol, tol_o, report=None):
    """Asserts the contract of a block SVD against the CONSTRUCTED values: per block max|s - s_b| <= tol max(s_b) and s
    descending, |(u s) vt - a|_F <= tol |a|_F, both factors isometries to tol_o, u and vt exactly zero outside their
    block's rows / columns.  ``report(figures)`` is called before anything is asserted; the figures are returned."""
    fig = svd_figures(a, blocks, u, s, vt, s_blocks)
    if report is not None:
        report(fig)
    assert fig["outside"] == 0, fig
    assert fig["descending"], fig
    assert fig["values"] <= tol, fig
    assert fig["zero_block_values"] == 0.0, fig
    assert fig["recon"] <= tol, fig
    assert fig["orth_u"] <= tol_o and fig["orth_vt"] <= tol_o, fig
    return fig


def widest(lds):
    """(Tc, Tr): the widest complex / real block the column kernel takes with ``lds`` bytes of dynamic LDS - pairs of
    8-column blocks of X and of V: 512 bytes per complex column, 256 per real one"""
    return lds // 512, lds // 256


def contract_tol(widths_and_heights):
    """The project's contract for the decomposition: 1e-13 while the widest block has fewer than 250 columns, 1e-12
    above (hundreds of rotations per column); isometries to 1e-12"""
    return (1e-13 if max(widths_and_heights) < 250 else 1e-12), 1e-12


def ragged_layout(T, last):
    """Five blocks of one call on the Gram path (an odd count: the done words are read back in pairs): heights, widths,
    spectra.  The widest keeps the launches going while the others converge in different sweeps; ``last`` is the
    spectrum of the 33 x 33 block."""
    return [T + 13, 150, 17, 9, 33], [T + 4, 70, 40, 1, 33], ["graded", "steps", "flat", [0.7], last]


def many_layout(rng, spec):
    """One 90 x 72 block and 119 blocks with heights and widths drawn from 1..6 (distinct random values)"""
    hs, ws = [90] + rng.integers(1, 7, 119).tolist(), [72] + rng.integers(1, 7, 119).tolist()
    sp = [spec] + [0.5 + rng.random(min(h, w)) for h, w in zip(hs[1:], ws[1:])]
    return hs, ws, sp


FULL_BLOCKS = [(40, 12, 28), (40, 12, 5), (12, 40, 12), (9, 9, 0), (1, 6, 5), (30, 30, 0)]    # (m, n, extra)
FULL_SPECTRA = ["graded", "steps", "graded", "flat", [0.3], "steps"]


def cases(lds):
    """{name: (seed, heights, widths, spectra, cplx)} of every matrix tests/test_block_svd_gpu.py decomposes, for a
    column kernel with ``lds`` bytes of dynamic LDS (rows = columns + 9 in the one-block cases: the cost is that of the
    square problem).  The read-back boundary (thousands of 2 x 2 blocks) is built by ``tiny_blocks``."""
    out = {}
    for cplx in (True, False):
        T = widest(lds)[0 if cplx else 1]
        t = "c128" if cplx else "f64"
        for spec in ("graded", "steps"):
            for name, n in (("gram+4", T + 4), ("gram+13", T + 13), ("top", T), ("slabs72", 72)) + \
                    ((("pass2-257", 257),) if cplx else ()):
                out[f"{name}-{spec}-{t}"] = (n, [n + 9], [n], [spec], cplx)
            out[f"many-{spec}-{t}"] = (120,) + tuple(many_layout(np.random.default_rng(120), spec)) + (cplx,)
        for last in ("graded", "zero"):
            out[f"ragged-{last}-{t}"] = (5,) + tuple(ragged_layout(T, last)) + (cplx,)
        out[f"full-{t}"] = (6, [b[0] for b in FULL_BLOCKS], [b[1] for b in FULL_BLOCKS], FULL_SPECTRA, cplx)
    return out


def build_case(case):
    """(a, blocks, s_blocks) of an entry of ``cases``"""
    seed, hs, ws, sp, cplx = case
    a, qnl, qnr, s_blocks = block_matrix(np.random.default_rng(seed), hs, ws, sp, cplx)
    return a, sector_blocks(qnl, qnr), s_blocks


def tiny_blocks(nblk):
    """``nblk`` real 2 x 2 blocks with distinct random values: (a, blocks, s_blocks)"""
    rng = np.random.default_rng(nblk)
    sp = [np.sort(0.1 + rng.random(2))[::-1] for _ in range(nblk)]
    a, qnl, qnr, s_blocks = block_matrix(rng, [2] * nblk, [2] * nblk, sp, False)
    return a, sector_blocks(qnl, qnr), s_blocks
