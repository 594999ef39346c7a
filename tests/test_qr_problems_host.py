"""The predictions of tests/test_block_qr_chol_gpu.py stand on their own (CPU, no engine): every block the GPU tests
send through the Cholesky-QR kernels is what tests/qr_problems.py claims - the singular values it was built with, and
under the float64 emulation of the device rule a decision that stays a factor MARGIN = 100 away from both thresholds
(n max|G - I| against 1e-9 and against 0.1) on the side its class claims, pivots of the last pass well inside the
window, every pivot positive.  This is a condition on the inputs: a draw that misses it is replaced in
``qr_problems.REDRAWN``, never excused.  The layouts have the block counts, extents and permutations they claim, the
heights the chunk counts the GPU test names, and the emulator's constants are those of the source."""
import os
import re

import numpy as np
import pytest

import qr_problems as qp            # (tests/qr_problems.py)

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "renormalizer_amd", "csrc", "mpse_cholqr.hip")


def _examine(cls, m, n, cplx, a=None):
    """(emulation, margins) of one block, after the checks every block has to pass"""
    tag = (cls, m, n, cplx)
    if a is None:
        a = qp.block(cls, m, n, cplx)
    assert a.shape == (m, n) and a.dtype == (complex if cplx else float), tag
    # the requested singular values: relative 1e-10 where float64 resolves them - LAPACK and the product U diag(s) V^H
    # both leave an absolute error of a few n u s_max (< 1e-13 s_max for n <= 256), which is all that can be asked of
    # the values below 1e-3 s_max of classes III and IV
    want = qp.spectrum(cls, n)
    got = np.linalg.svd(a, compute_uv=False)
    assert np.all(np.abs(got - want) <= 1e-10 * want + 1e-13 * want[0]), (tag, np.abs(got / want - 1).max())
    em = qp.emulate(a)
    mg = qp.margins(cls, em)
    shifted, passes, first = qp.CLAIMS[cls]
    assert (em["shifted"] > 0, em["passes"], em["first_order"]) == (shifted, passes, first), (tag, em)
    assert em["positive"], (tag, "a pivot of the emulation is not positive")
    for what, v in mg.items():
        assert v >= qp.MARGIN, (tag, what, v, em)
    if not shifted:     # "no pivot shifted" is a claim too: the smallest pivot keeps 100 theta of its diagonal entry
        assert em["pivot_ratio"] >= qp.MARGIN * qp.THETA, (tag, em["pivot_ratio"])
        mg = dict(mg, **{"pivot ratio above theta": em["pivot_ratio"] / qp.THETA})
    if em["pivots"] is not None:      # the window guards whichever pass is the last; these sit within 1e-3 of 1
        assert qp.WINDOW[0] * 2 < em["pivots"].min() and em["pivots"].max() < qp.WINDOW[1] / 2, (tag, em["pivots"])
        assert np.abs(em["pivots"] - 1).max() < 1e-3, (tag, em["pivots"])
    assert em["orth"] < 1e-14, (tag, em["orth"])      # the emulated rule itself delivers an isometry
    return em, mg


@pytest.fixture(scope="module")
def examined():
    """(class, m, n, cplx) -> (emulation, margins), each block built and emulated once"""
    done = {}

    def get(cls, m, n, cplx):
        key = (cls, m, n, cplx)
        if key not in done:
            done[key] = _examine(*key)
        return done[key]
    return get


def _all_blocks():
    out = [(cls, m, n) for n in qp.WIDTHS for cls, m in qp.single_cases(n)]
    out += [(cls, m, n) for m, n, cls in qp.MIXED]
    out += [("II", 300, 257)]
    return out


def test_emulator_constants_are_those_of_the_source():
    src = open(SRC).read()
    assert re.search(r'getenv\("MPSE_CHOLQR_THETA"\);\s*return e \? atof\(e\) : 1e-12;', src)
    assert re.search(r'getenv\("MPSE_CHOLQR_TAU"\);\s*return e \? atof\(e\) : 0\.1;', src)
    assert (qp.THETA, qp.TAU, qp.FIRST_ORDER, qp.WINDOW) == (1e-12, 0.1, 1e-9, (0.25, 4.0))
    # both factor kernels: the first-order threshold, the shift, the done rule; the window of panel_eliminate
    assert src.count("if (pass >= 2 && (double)nn * maxdev <= 1e-9) {") == 2
    assert src.count("11.0 * ((double)B.mm * nn + (double)nn * (nn + 1)) * 1.1102230246251565e-16 * trace") == 2
    assert src.count("pass == 3 || (pass == 2 && (double)nn * maxdev <= tau)") == 2
    assert "if (window && !(d >= 0.25 && d <= 4.0)) ok = false;" in src
    assert "if (dyn) piv = piv > thr[k] ? piv : piv + sDinv[16];" in src
    assert "if (max_P <= 10)" in src and qp.RL_MAX_COLS == 160 and qp.UNIT == 1.1102230246251565e-16
    assert "if (rpc < 32) rpc = 32;" in src and qp.RPC == 32
    assert "blks[b].nn > 256) return false;" in src and qp.MAX_COLS == 256
    with pytest.raises(AssertionError):
        qp.emulate(np.eye(3), theta=0.0)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("n", qp.WIDTHS)
def test_single_block_cases_keep_their_margins(examined, n, cplx):
    cases = qp.single_cases(n)
    assert len(cases) == 3 * (1 if n == 1 else 5)
    for cls, m in cases:
        examined(cls, m, n, cplx)


@pytest.mark.parametrize("cplx", [True, False])
def test_mixed_call_blocks_keep_their_margins(examined, cplx):
    for m, n, cls in qp.MIXED:
        examined(cls, m, n, cplx)
    examined("II", 300, 257, cplx)        # the block one column too wide for the path: a sound block all the same
    # the fallback case: the zeroed column leaves pass 2 a zero pivot - the emulation flags it as the device has to
    b, j = qp.MIXED_ZERO_COLUMN
    m, n, cls = qp.MIXED[b]
    a = qp.block(cls, m, n, cplx)
    a[:, j] = 0
    em = qp.emulate(a)
    assert not em["positive"] and em["shifted"] >= 1 and em["dev2"] >= 100 * qp.TAU, em


def test_smallest_margin_is_the_recorded_one(examined):
    """over every block of every GPU case, both dtypes: printed, >= MARGIN, and no smaller than qr_problems records"""
    worst = {}
    for cplx in (True, False):
        for cls, m, n in _all_blocks():
            for what, v in examined(cls, m, n, cplx)[1].items():
                key = ("I" if cls == "Is" else cls, what)
                if v < worst.get(key, (np.inf,))[0]:
                    worst[key] = (v, (cls, m, n, cplx))
    for key in sorted(worst):
        print(f"\n[qr_problems] class {key[0]:3s} {key[1]:32s} {worst[key][0]:9.2e}  at {worst[key][1]}", end="")
    smallest = min(v for v, _ in worst.values())
    print(f"\n[qr_problems] smallest margin {smallest:.3e}")
    assert smallest >= qp.MARGIN
    assert qp.MARGIN_MEASURED * 0.9 <= smallest <= qp.MARGIN_MEASURED * 1.1, (smallest, qp.MARGIN_MEASURED)


def test_heights_and_chunks():
    for n in qp.WIDTHS:
        groups = qp.super_tiles([n])
        sq, odd, tall = qp.heights(n)
        assert sq == n and n < odd <= n + 2 and odd % 4 != 0 and n <= tall <= 700 and tall % 16 != 0
        for m in (sq, odd, tall):
            nch, rpc = qp.chunks(m, 256, groups)
            assert rpc == qp.RPC and nch == -(-m // 32)
        assert odd % 32 != 0                                        # a partly filled last chunk
        nch = qp.chunks(tall, 256, groups)[0]
        assert nch % 4 != 0 and (nch in (5, 6, 7) if n < 255 else nch in (21, 22))      # a ragged last macro chunk
    assert {qp.chunks(qp.TALL[n])[0] for n in qp.WIDTHS if n < 255} == {5, 6, 7}
    # the mixed call: 30 super-tiles, 32 rows per chunk for every block
    ws = [n for _, n, _ in qp.MIXED]
    assert qp.super_tiles(ws) == 30
    assert [qp.chunks(m, 256, 30) for m, _, _ in qp.MIXED] == [(2, 32), (2, 32), (4, 32), (10, 32), (2, 32), (1, 32)]
    # the rule itself, at the headline's shape: 2 blocks of 145 and 111 columns on 256 compute units
    assert qp.super_tiles([145, 111]) == 25 and qp.chunks(2816, 256, 25) == (64, 44)
    assert qp.classes_of(1) == ("I",) and qp.classes_of(15) == qp.CLASSES


def test_predictions():
    ws, cs = [n for _, n, _ in qp.MIXED], [c for _, _, c in qp.MIXED]
    assert tuple(qp.predict(ws, cs).values()) == (1, 0, 1, 0, 6, 4, 2, 1)
    keep = [i for i, w in enumerate(ws) if w <= 160]
    assert tuple(qp.predict([ws[i] for i in keep], [cs[i] for i in keep]).values()) == (1, 1, 0, 0, 5, 4, 2, 1)
    assert tuple(qp.predict([160], ["III"]).values()) == (1, 1, 0, 0, 1, 0, 0, 1)
    assert tuple(qp.predict([161], ["Is"]).values()) == (1, 0, 1, 0, 1, 1, 1, 0)
    assert tuple(qp.predict([17], ["IV"]).values()) == (1, 1, 0, 0, 1, 0, 0, 0)
    assert tuple(qp.predict([17], ["II"]).values()) == (1, 1, 0, 0, 1, 1, 0, 0)
    assert tuple(qp.NO_CHANGE) == qp.STAT_NAMES and not any(qp.NO_CHANGE.values())


@pytest.mark.parametrize("cplx", [True, False])
def test_layouts(cplx):
    for wide, zero in ((True, False), (False, False), (True, True)):
        a, blocks, ws, cs = qp.mixed(cplx, wide=wide, zero_column=zero)
        spec = [s for s in qp.MIXED if wide or s[1] <= 160]
        assert len(blocks) == len(spec) == (6 if wide else 5) and ws == [s[1] for s in spec] and cs == [s[2] for s in spec]
        assert a.shape == (sum(s[0] for s in spec), sum(s[1] for s in spec)) and a.dtype == (complex if cplx else float)
        assert [(len(r), len(c)) for r, c in blocks] == [s[:2] for s in spec]
        rows, roff, cols, coff = qp.offsets(blocks)
        assert rows.dtype == cols.dtype == roff.dtype == coff.dtype == np.int64
        assert np.array_equal(np.sort(rows), np.arange(a.shape[0])) and np.array_equal(np.sort(cols), np.arange(a.shape[1]))
        assert not np.array_equal(rows, np.arange(a.shape[0])) and not np.array_equal(cols, np.arange(a.shape[1]))   # permuted
        assert roff.tolist() == np.cumsum([0] + [s[0] for s in spec]).tolist()
        assert coff.tolist() == np.cumsum([0] + [s[1] for s in spec]).tolist()
        mask = np.zeros(a.shape, dtype=bool)
        for b, (r, c) in enumerate(blocks):
            assert np.all(np.diff(r) > 0) and np.all(np.diff(c) > 0)
            assert r.max() - r.min() >= len(r) or len(r) == a.shape[0]          # interleaved with the other blocks
            mask[np.ix_(r, c)] = True
            want = qp.block(spec[b][2], spec[b][0], spec[b][1], cplx)
            if zero and b == qp.MIXED_ZERO_COLUMN[0]:
                assert not np.any(a[np.ix_(r, c)][:, qp.MIXED_ZERO_COLUMN[1]])
                want[:, qp.MIXED_ZERO_COLUMN[1]] = 0
            assert np.array_equal(a[np.ix_(r, c)], want)
        assert not np.any(a[~mask])
        x, xb = qp.adjoint(a, blocks)
        assert x.flags.c_contiguous and np.array_equal(x, a.conj().T)
        assert all(np.array_equal(r2, c) and np.array_equal(c2, r) for (r, c), (r2, c2) in zip(blocks, xb))
    a, blocks, ws, cs = qp.single("III", 40, 17, cplx)
    assert a.shape == (40, 17) and ws == [17] and cs == ["III"] and len(blocks) == 1
    assert np.array_equal(blocks[0][0], np.arange(40)) and np.array_equal(blocks[0][1], np.arange(17))
    assert np.array_equal(a, qp.block("III", 40, 17, cplx))                      # the same block for the same arguments
