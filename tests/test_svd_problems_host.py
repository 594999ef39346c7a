"""The references of tests/test_block_svd_gpu.py stand on their own (CPU, no engine): the constructed singular systems
of tests/svd_problems.py are what they claim to be, LAPACK meets ``check_svd`` at 1e-13 on every matrix the GPU tests
decompose - so the bounds asked of the kernels (1e-13 / 1e-12) are not bounds on the construction - and ``check_svd``
refuses factors that are wrong in each of the ways it names."""
import numpy as np
import pytest

import svd_problems as sp            # (tests/svd_problems.py)

LDS = (150 * 1024, 64 * 1024)        # what the column kernel is granted, and what a runtime that refuses leaves it


def test_named_spectra():
    for k in (11, 72, 304):
        g, st = sp.spectrum("graded", k), sp.spectrum("steps", k)
        for s in (g, st):
            assert s.shape == (k,) and np.all(np.diff(s) <= 0) and np.all(s[-5:] == 0) and np.all(s[:-5] > 0)
        assert g[0] == 1.0 and np.array_equal(g[:-5], np.exp(-30.0 * np.arange(k - 5) / k))
        assert np.array_equal(st[:k - 5], 2.0 ** -(np.arange(k - 5) // 8))       # clusters of 8 equal values
    assert np.all(sp.spectrum("graded", 9) > 0) and np.all(sp.spectrum("steps", 10) > 0)     # no rank deficit up to 10
    assert np.array_equal(sp.spectrum("flat", 7), np.ones(7)) and not np.any(sp.spectrum("zero", 7))
    assert np.array_equal(sp.spectrum([0.2, 0.9], 2), [0.9, 0.2])


@pytest.mark.parametrize("cplx", [False, True])
def test_block_matrix_structure(cplx):
    rng = np.random.default_rng(1)
    hs, ws, spec = [13, 4, 6, 1], [11, 9, 6, 3], ["graded", "steps", "flat", "zero"]
    a, qnl, qnr, s_blocks = sp.block_matrix(rng, hs, ws, spec, cplx)
    assert a.shape == (24, 29) and a.dtype == (complex if cplx else float) and qnl.shape == (24, 1) and qnr.shape == (29, 1)
    assert not np.array_equal(qnl[:, 0], np.sort(qnl[:, 0]))                     # permuted
    blocks = sp.sector_blocks(qnl, qnr)
    assert [(len(ls), len(rs)) for ls, rs in blocks] == list(zip(hs, ws))
    mask = np.zeros(a.shape, dtype=bool)
    for b, (ls, rs) in enumerate(blocks):
        assert np.all(qnl[ls, 0] == b) and np.all(qnr[rs, 0] == -b) and np.all(np.diff(ls) > 0) and np.all(np.diff(rs) > 0)
        mask[np.ix_(ls, rs)] = True
        sv = np.linalg.svd(a[np.ix_(ls, rs)], compute_uv=False)
        assert np.abs(sv - s_blocks[b]).max() <= 1e-14
    assert not np.any(a[~mask])
    g = a[np.ix_(*blocks[2])]                                                    # flat: orthonormal columns already
    assert np.abs(g.conj().T @ g - np.eye(6)).max() < 1e-14
    assert not np.any(a[np.ix_(*blocks[3])])
    rows, roff, cols, coff = sp.offsets(blocks)
    assert roff.tolist() == [0, 13, 17, 23, 24] and coff.tolist() == [0, 11, 20, 26, 29]
    assert sorted(rows.tolist()) == list(range(24)) and sorted(cols.tolist()) == list(range(29))
    a2, ql2, _, _ = sp.block_matrix(np.random.default_rng(1), hs, ws, spec, cplx, permute=False)
    assert np.array_equal(ql2[:, 0], np.sort(ql2[:, 0])) and np.any(a2[:13, :11]) and not np.any(a2[:13, 11:])


def test_widths_follow_the_granted_lds():
    assert sp.widest(150 * 1024) == (300, 600) and sp.widest(64 * 1024) == (128, 256)
    assert sp.contract_tol([249, 9]) == (1e-13, 1e-12) and sp.contract_tol([250]) == (1e-12, 1e-12)
    c = sp.cases(150 * 1024)
    assert c["gram+13-steps-c128"][1:3] == ([322], [313]) and c["gram+4-graded-f64"][1:3] == ([613], [604])
    assert c["ragged-zero-f64"][1:3] == ([613, 150, 17, 9, 33], [604, 70, 40, 1, 33])
    assert len(c["many-graded-c128"][1]) == 120 and max(c["many-graded-c128"][1][1:]) <= 6
    assert sp.cases(64 * 1024)["top-steps-c128"][2] == [128]


@pytest.mark.parametrize("lds", LDS)
def test_lapack_meets_the_contract_on_every_case(lds):
    """np.linalg.svd of every matrix of the GPU tests is within 1e-13 of the constructed values, reconstructs to 1e-13
    and is an isometry to 1e-13 (measured: 2e-15, 5e-15, 4e-15 at 313 complex / 613 real columns)"""
    worst = {"values": 0.0, "recon": 0.0, "orth_u": 0.0, "orth_vt": 0.0}
    for name, case in sp.cases(lds).items():
        if lds != LDS[0] and not name.startswith(("gram", "top", "ragged")):
            continue                                             # (the other layouts do not depend on the LDS)
        a, blocks, s_blocks = sp.build_case(case)
        u, s, vt = sp.lapack_svd(a, blocks)
        fig = sp.check_svd(a, blocks, u, s, vt, s_blocks, 1e-13, 1e-13)
        for k in worst:
            worst[k] = max(worst[k], fig[k])
    print("LAPACK, worst over the cases:", worst)


@pytest.mark.parametrize("nblk", [2000, 2001])
def test_lapack_meets_the_contract_on_tiny_blocks(nblk):
    a, blocks, s_blocks = sp.tiny_blocks(nblk)
    assert a.shape == (2 * nblk, 2 * nblk) and len(blocks) == nblk
    u, s, vt = sp.lapack_svd(a, blocks)
    sp.check_svd(a, blocks, u, s, vt, s_blocks, 1e-13, 1e-13)


def test_check_svd_refuses_wrong_factors():
    a, blocks, s_blocks = sp.build_case(sp.cases(LDS[0])["full-c128"])
    u, s, vt = sp.lapack_svd(a, blocks)
    seen = []
    fig = sp.check_svd(a, blocks, u, s, vt, s_blocks, 1e-13, 1e-13, report=seen.append)
    assert seen == [fig]
    K = len(s)

    def refused(u2, s2, vt2, sb=s_blocks):
        with pytest.raises(AssertionError):
            sp.check_svd(a, blocks, u2, s2, vt2, sb, 1e-13, 1e-13)

    s2 = s.copy()
    s2[3] += 2e-13                                   # a value off by more than tol (the block's largest value is 1)
    refused(u, s2, vt)
    s2 = s.copy()
    s2[[0, 1]] = s2[[1, 0]]                          # not descending inside the block
    u2, vt2 = u.copy(), vt.copy()
    u2[:, [0, 1]], vt2[[0, 1]] = u2[:, [1, 0]], vt2[[1, 0]]
    refused(u2, s2, vt2)
    u2 = u.copy()
    u2[:, 0] *= 1 + 1e-12                            # no isometry (and no reconstruction)
    refused(u2, s, vt)
    vt2 = vt.copy()
    vt2[K - 1] *= 1 + 1e-12                          # a right vector of a ZERO value: only the isometry check sees it
    refused(u, s, vt2)
    u2 = u.copy()
    outside = np.setdiff1d(np.arange(a.shape[0]), blocks[0][0])
    u2[outside[0], 0] = 1e-300                       # an entry outside the block's rows, however small
    refused(u2, s, vt)
    th = 1e-6                                        # a rotation inside the block by 1e-6: isometries, wrong reconstruction
    u2 = u.copy()
    u2[:, 0], u2[:, 1] = np.cos(th) * u[:, 0] - np.sin(th) * u[:, 1], np.sin(th) * u[:, 0] + np.cos(th) * u[:, 1]
    refused(u2, s, vt)
    # a zero block must come back as zeros
    a0, blocks0, sb0 = sp.build_case(sp.cases(LDS[0])["ragged-zero-f64"])
    u0, s0, vt0 = sp.lapack_svd(a0, blocks0)
    sp.check_svd(a0, blocks0, u0, s0, vt0, sb0, 1e-13, 1e-13)
    s0[-1] = 1e-300
    with pytest.raises(AssertionError):
        sp.check_svd(a0, blocks0, u0, s0, vt0, sb0, 1e-13, 1e-13)
