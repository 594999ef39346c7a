"""Host side of the canonicalise / compress tests (no GPU): the helpers of tests/compress_refs.py against the dense
wavefunction, the block kinds the fixtures put in front of the kernels, and - for every fixture and seed that
tests/test_compress_gpu.py uses - the conditions that keep its comparisons of truncated states away from near-ties:
every cut has a gap (s[m - 1] - s[m]) / s[0] of at least 1e-3 and every threshold count a margin of at least 1e-3.
These are statements about the oracle's own values; the GPU file asserts them again before it compares anything."""
import numpy as np
import pytest

import compress_refs as R                               # (tests/compress_refs.py)
from oracle import mps_oracle as orc


def _pairs(cases):
    """(fixture, cplx, seed) of every case of a table of compress_refs"""
    return [(c[0], cplx, c[1 + cplx]) for c in cases for cplx in (False, True) if c[1 + cplx] is not None]


ALL = [(n, c) for n in R.FIXTURES for c in (False, True) if c or n not in R.COMPLEX_ONLY]


@pytest.mark.parametrize("name, cplx", ALL)
def test_chain_structure(name, cplx):
    """normal entries where label_l + sigma == label_r and exact zeros elsewhere, the convention of ``Mps.random``, the
    real part drawn before the imaginary one, bonds of at most 40 (96 in the wide chains), a state that is not zero"""
    sigmaqn, bond_qn, decay = R.FIXTURES[name]
    st = R.fixture(name, 5, cplx)
    assert st.qnidx == st.nsite - 1 and st.to_right is False and np.array_equal(st.qn[-1], [[0]])
    assert st.bond_dims == [len(b) for b in bond_qn]
    assert max(st.bond_dims) <= (96 if name in R.COMPLEX_ONLY else 40)
    left = [np.asarray(b).reshape(-1, 1) for b in bond_qn]
    for i, a in enumerate(st.sites):
        assert np.iscomplexobj(a) == cplx
        allowed = (left[i][:, None, None, 0] + np.asarray(sigmaqn[i])[None, :, None, 0] == left[i + 1][None, None, :, 0])
        assert np.all(a[~allowed] == 0) and np.all(a[allowed] != 0)
    rng = np.random.default_rng(5)
    drawn = [rng.standard_normal(st.sites[0].shape) for _ in range(1 + cplx)]
    scale = 1.0 if decay is None else decay ** np.arange(st.sites[0].shape[2])
    first = (drawn[0] + 1j * drawn[1] if cplx else drawn[0]) * (st.sites[0] != 0) * scale
    assert np.array_equal(st.sites[0], first)
    assert np.linalg.norm(R.dense(st)) > 0
    # the labels of the total: every amplitude of the dense state carries the total charge
    psi = R.dense(st)
    charge = np.zeros(psi.shape, dtype=int)
    for i, s in enumerate(sigmaqn):
        charge = charge + np.asarray(s)[:, 0].reshape([-1 if k == i else 1 for k in range(psi.ndim)])
    assert np.all(psi[charge != st.qntot[0]] == 0)


def test_labels_are_those_of_the_model():
    for nmol in (2, 3):
        model = R.holstein_model(nmol)
        assert model.pbond_list == list(R.HOLSTEIN_D * nmol) and model.qn_size == 1
        for b, s in zip(model.basis, R.holstein_sigmaqn(nmol)):
            assert np.array_equal(np.asarray(b.sigmaqn).reshape(b.nbas, -1), s)
    m = R.chain_model(R.nosym_sigmaqn())
    assert m.pbond_list == list(R.HOLSTEIN_D * 3) and m.nsite == 9 and m.qn_size == 1


def test_ragged_chain_puts_every_block_kind_in_one_sweep():
    """The right-going SVD sweep over the canonicalised ``ragged`` chain: a 1 x 1 block, a block wider than tall (the
    adjoint path) whose width is no multiple of 16 and rows without a partner column in ONE decomposition (site 3);
    single-column blocks and blocks taller than wide at its neighbours.  The QR sweep before it has blocks of one row
    and blocks wider and taller than wide."""
    st = R.fixture("ragged", 1, False)
    qr = R.sweep_blocks(st, orc.canonicalise)
    assert qr[2] == (6, [(5, 7), (9, 7)], 0) and qr[3] == (5, [(1, 15), (30, 21)], 0) and qr[4] == (4, [(1, 4), (19, 84)], 0)
    svd = R.sweep_blocks(st, lambda s: orc.compress(s, "fixed", max_dims=[10 ** 6] * 10))
    assert svd[0] == (0, [(1, 1), (1, 1)], 0)
    assert svd[2] == (2, [(9, 1), (12, 11)], 0)
    assert svd[3] == (3, [(1, 1), (12, 19)], 11)
    assert svd[4] == (4, [(4, 1), (48, 21)], 0)
    assert svd[5] == (5, [(3, 5), (63, 7)], 0) and svd[6] == (6, [(10, 7)], 10)
    back = R.sweep_blocks(st, lambda s: orc.compress(s, "fixed", max_dims=[10 ** 6] * 10))
    assert back[3] == (5, [(1, 9), (21, 21)], 0) and back[4] == (4, [(1, 4), (12, 84)], 0)


def test_wide_chains_have_blocks_of_more_than_64_columns():
    for name, seed in (("holstein_wide", 3), ("nosym_wide", 4)):
        st = R.fixture(name, seed, True)
        qr = R.sweep_blocks(st, orc.canonicalise)
        svd = R.sweep_blocks(st, lambda s: orc.compress(s, "fixed", max_dims=[10 ** 6] * 10))
        svd += R.sweep_blocks(st, lambda s: orc.compress(s, "fixed", max_dims=[10 ** 6] * 10))
        assert max(r for _, blocks, _ in qr for r, c in blocks) >= 70
        # the smaller side: 192 x 72 without a symmetry; 24 x 144 (going left) is the widest of the Holstein chain
        assert max(min(r, c) for _, blocks, _ in svd for r, c in blocks) == (72 if name == "nosym_wide" else 36)
        assert max(c for _, blocks, _ in svd for r, c in blocks) == (288 if name == "nosym_wide" else 144)


@pytest.mark.parametrize("name, cplx, seed", _pairs(R.EXACT_CASES))
def test_sweeps_without_truncation_keep_the_dense_state(name, cplx, seed):
    """the oracle's canonicalise (both directions) and compress without truncation leave ``dense`` alone to 1e-13, leave
    isometries behind, and ``compress`` returns the dense Schmidt values at every bond"""
    st = R.fixture(name, seed, cplx)
    psi = R.dense(st)
    for start in ("right", "left"):
        can = R.canonical(st, start)
        assert R.rel(R.dense(can), psi) < 1e-13 and R.isometry_error(can.sites, can.qnidx) < 1e-13
        out = can.copy()
        _, s_list = orc.compress(out, "fixed", max_dims=[10 ** 6] * (st.nsite + 1))
        assert R.rel(R.dense(out), psi) < 1e-13 and R.isometry_error(out.sites, out.qnidx) < 1e-13
        bonds = range(1, st.nsite) if start == "right" else range(st.nsite - 1, 0, -1)
        for k, (bond, s) in enumerate(zip(bonds, s_list), 1):
            ref = R.schmidt_values(psi, bond)
            w = min(len(s), len(ref))
            assert np.all(np.diff(s) <= 0)
            assert np.abs(s[:w] - ref[:w]).max() < k * 1e-13 * ref[0]
            assert np.all(s[w:] < k * 1e-13 * ref[0]) and np.all(ref[w:] < k * 1e-13 * ref[0])


def test_direct_sum_fold_and_operator_twins():
    a, b = R.fixture("holstein_small", 11, True), R.fixture("holstein_small", 12, True)
    a.coeff, b.coeff = 0.5j, 2.0
    assert R.rel(R.dense(R.direct_sum(a, b)), R.dense(a) + R.dense(b)) < 1e-14
    a.coeff = b.coeff = 1.5
    s = R.direct_sum(a, b)
    assert s.coeff == 1.5 and R.rel(R.dense(s), R.dense(a) + R.dense(b)) < 1e-14
    assert s.bond_dims[1:-1] == [x + y for x, y in zip(a.bond_dims[1:-1], b.bond_dims[1:-1])]
    # a density operator: the folded chain has the dense operator's entries, re-ordered
    from renormalizer_amd import Mpo
    st = R.fixture("holstein6", 25, False)
    mpo = Mpo(R.holstein_model(2))
    h = mpo.todense()
    ds = list(R.HOLSTEIN_D * 2)
    rho = R.diagonal_operator(st)
    full = np.diag(R.dense(st).ravel())
    assert np.array_equal(R.dense(R.folded(rho)), R.fold_dense_operator(full, ds))
    prod = R.operator_reference(mpo, rho)[0]
    assert prod.sites[0].ndim == 3 and prod.sigmaqn[0].shape == (4, 1)
    assert R.rel(R.dense(prod), R.fold_dense_operator(h @ full, ds)) < 1e-13
    # a pure state
    ket = R.operator_reference(mpo, st)[0]
    assert R.rel(R.dense(ket).ravel(), h @ R.dense(st).ravel()) < 1e-13
    assert ket.bond_dims == [x * y for x, y in zip(st.bond_dims, mpo.bond_dims)]


@pytest.mark.parametrize("start", ("right", "left"))
@pytest.mark.parametrize("name, cplx, seed", _pairs(R.EY_CASES))
def test_one_bond_truncation_is_eckart_young(name, cplx, seed, start):
    """a sweep that cuts one bond of a canonical state gives the best approximation of that Schmidt rank; the gap at
    each of the bonds tests/test_compress_gpu.py cuts is at least 1e-3"""
    can = R.canonical(R.fixture(name, seed, cplx), start)
    psi = R.dense(can)
    for bond, m in R.EY_BONDS:
        s = R.schmidt_values(psi, bond)
        gap = (s[m - 1] - s[m]) / s[0]
        assert gap >= R.MIN_GAP
        trunc = [np.inf] * (can.nsite + 1)
        trunc[bond] = m
        out = can.copy()
        orc.compress(out, temp_m_trunc=[10 ** 6 if np.isinf(t) else t for t in trunc])
        assert out.bond_dims[bond] == m
        assert R.rel(R.dense(out), R.best_rank_at_bond(psi, bond, m)) < 1e-13 / gap


@pytest.mark.parametrize("start", ("right", "left"))
@pytest.mark.parametrize("criteria", ("fixed", "threshold", "both"))
@pytest.mark.parametrize("name, cplx, seed", _pairs(R.TRUNC_CASES))
def test_truncation_cases_meet_the_conditions(name, cplx, seed, criteria, start):
    ref = R.truncation_reference(R.fixture(name, seed, cplx), criteria, start)
    g1, g2 = R.assert_conditions(ref)
    print(f"{name} cplx={cplx} {criteria} {start}: gaps {g1:.1e} {g2:.1e}, margin {ref.margin}, "
          f"bonds {ref.first.bond_dims} -> {ref.second.bond_dims}")
    if criteria != "threshold":
        assert max(ref.first.bond_dims) == R.M1
    assert max(ref.second.bond_dims) == R.M2


@pytest.mark.parametrize("name, cplx, seeds", [(c[0], cplx, c[1 + cplx]) for c in R.SUM_CASES for cplx in (False, True)])
def test_sum_cases_meet_the_conditions(name, cplx, seeds):
    """a + a has the Schmidt ranks of a at every bond, which are the bond dimensions of the canonicalised a; the
    smallest value kept is 1e-3 of the largest, the threshold of 1e-8 far from every value"""
    a = R.fixture(name, seeds[0], cplx)
    dims = R.canonical(a, "right").bond_dims
    psi = R.dense(a)
    spectra = [R.schmidt_values(psi, b) for b in range(1, a.nsite)]
    ranks = [1] + [int(np.sum(s > 1e-10 * s[0])) for s in spectra] + [1]
    assert dims == ranks
    can = R.canonical(R.direct_sum(a, a), "right")
    assert can.bond_dims != dims
    out = can.copy()
    _, s = orc.compress(out, "threshold", 1e-8)
    assert out.bond_dims == dims
    gaps = R.cut_gaps(s, R.kept_dims(out, True))
    assert gaps and min(gaps) >= R.MIN_GAP and R.threshold_margin(s, 1e-8) >= R.MIN_MARGIN
    assert all(np.all(x[m:] < 1e-13 * x[0]) for x, m in zip(s, dims[1:-1]))
    assert R.rel(R.dense(out), 2 * psi) < len(gaps) * 1e-13 / min(gaps)


@pytest.mark.parametrize("cplx", (False, True))
def test_operator_cases_meet_the_conditions(cplx):
    from renormalizer_amd import Mpo
    model = R.holstein_model()
    for name, op, *seeds in R.OP_CASES:
        mpo = Mpo(model) if op == "H" else Mpo.onsite(model, r"a^\dagger")
        st = R.fixture(name, seeds[cplx], cplx)
        prod, _, out, s, gaps = R.operator_reference(mpo, st)
        assert prod.qntot[0] == st.qntot[0] + (op != "H")
        assert gaps and min(gaps) >= R.MIN_GAP and max(out.bond_dims) == R.OP_M, (name, gaps)
    name, *seeds = R.MPDM_CASE
    rho = R.diagonal_operator(R.fixture(name, seeds[cplx], cplx))
    _, _, out, s, gaps = R.operator_reference(Mpo(R.holstein_model(2)), rho)
    assert gaps and min(gaps) >= R.MIN_GAP and max(out.bond_dims) == R.OP_M, (name, gaps)
