"""``Mps.canonicalise``, ``Mps.compress``, ``Mps.add`` + compression, ``compressed_sum``, ``Mpo.contract(algo="svd")``
and the same sweeps over an ``MpDm`` against two references: the oracle's NumPy sweeps (oracle/mps_oracle.py) and the
dense wavefunction (Schmidt values and Eckart-Young truncations by ``numpy.linalg.svd``).  The chains come from
tests/compress_refs.py: real quantum numbers, ragged blocks, default kernel paths only.

Bounds, EPS = 1e-13 being the bound of the block QR / block SVD tests for blocks of this size:
  * a sweep that truncates nothing leaves the dense state alone to EPS (relative, 2-norm) and leaves isometries
    behind to EPS (largest entry of A^H A - 1);
  * singular values: k EPS s[0] at the k-th bond since the canonical input (Weyl, one backward error per bond passed);
  * truncated states and the Eckart-Young check: n_cut EPS / g relative to the norm, n_cut the number of bonds cut so far
    and g the smallest gap (s[m - 1] - s[m]) / s[0] at a cut, from the reference's spectra (Wedin); g >= 1e-3 is
    asserted first, as tests/test_compress_refs_host.py does on the CPU.
Integers (bond dimensions, qnidx, to_right, labels) are compared exactly; where singular values can tie (zeros of a
rank-deficient bond) or a truncation follows, the labels of a bond as sorted multisets.  Every test prints the worst
ratio of a figure to its bound."""
import functools

import numpy as np
import pytest

import compress_refs as R                               # (tests/compress_refs.py)
from oracle import mps_oracle as orc
from renormalizer_amd import CompressConfig
from renormalizer_amd.mps import MpDm, Mpo, Mps
from renormalizer_amd.mps.mps import compressed_sum

pytestmark = pytest.mark.gpu

EPS = 1e-13


def _pairs(cases):
    return [(c[0], cplx, c[1 + cplx]) for c in cases for cplx in (False, True) if c[1 + cplx] is not None]


@functools.lru_cache(maxsize=None)
def _model(name):
    sigmaqn = R.FIXTURES[name][0]
    return R.chain_model(sigmaqn) if name.startswith("nosym") else R.holstein_model(len(sigmaqn) // 3)


class _Figures:
    """figures with their bounds: collected, the worst ratio printed, then all asserted"""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def add(self, what, value, bound):
        self.rows.append((float(value) / bound, what, float(value), bound))

    def done(self):
        worst = max(self.rows)
        print(f"{self.tag}: worst ratio to its bound {worst[0]:.2e} ({worst[1]}: {worst[2]:.2e} / {worst[3]:.2e}; "
              f"{len(self.rows)} figures)")
        bad = [r for r in self.rows if not r[0] < 1]
        assert not bad, bad


def _labels(qn, exact):
    qn = [np.asarray(q).reshape(-1).tolist() for q in qn]
    return qn if exact else [sorted(q) for q in qn]


def _same_bookkeeping(mps, ref, exact):
    assert mps.bond_dims == ref.bond_dims
    assert (mps.qnidx, mps.to_right) == (ref.qnidx, ref.to_right)
    assert np.array_equal(mps.qntot, ref.qntot)
    assert _labels(mps.qn, exact) == _labels(ref.qn, exact)


def _same_spectra(fig, rows, s_ref, k0=0):
    """rows: what ``compress(ret_s=True)`` returned; s_ref: the reference's values per decomposition; the k-th
    decomposition of this sweep is the (k0 + k)-th bond since the canonical input"""
    assert len(rows) == len(s_ref)
    for k, (row, ref) in enumerate(zip(rows, s_ref), 1):
        assert np.all(row[len(ref):] == 0) and np.all(np.diff(row) <= 0)
        w = min(len(row), len(ref))
        fig.add(f"sigma, decomposition {k}", np.abs(row[:w] - ref[:w]).max(), (k0 + k) * EPS * ref[0])
        if w < len(ref):
            fig.add(f"sigma beyond the row, decomposition {k}", np.abs(ref[w:]).max(), (k0 + k) * EPS * ref[0])


def _fixed(m, dims=None):
    cfg = CompressConfig("fixed", max_bonddim=m)
    if dims is not None:
        cfg.max_dims = np.array(dims, dtype=int)
    return cfg


@pytest.mark.parametrize("name, cplx, seed", _pairs(R.EXACT_CASES))
def test_canonicalise(name, cplx, seed):
    """From the last site to the left, then back to the right: the dense state and isometries to EPS; bond
    dimensions, qnidx, to_right and every label list equal to the oracle's as lists; a real chain stays float64.
    Observed on MI355X: worst ratio 0.03 (dense state 2.95e-15, the chain with the bond of 96)."""
    st = R.fixture(name, seed, cplx)
    psi = R.dense(st)
    mps = R.to_device(_model(name), st)
    fig = _Figures(f"canonicalise {name} cplx={cplx}")
    for centre in (0, st.nsite - 1):
        assert mps.canonicalise() is mps
        orc.canonicalise(st)
        assert mps.qnidx == centre
        _same_bookkeeping(mps, st, exact=True)
        arrays = mps.to_arrays()
        assert mps.dtype == np.dtype(complex if cplx else float) and all(a.dtype == mps.dtype for a in arrays)
        fig.add(f"dense, centre {centre}", R.rel(mps.todense(), psi), EPS)
        fig.add(f"isometries, centre {centre}", R.isometry_error(arrays, centre), EPS)
        fig.add(f"sites against the oracle's dense, centre {centre}", R.rel(mps.todense(), R.dense(st)), EPS)
    fig.done()


@pytest.mark.parametrize("start", ("right", "left"))
@pytest.mark.parametrize("name, cplx, seed", _pairs(R.EXACT_CASES))
def test_compress_without_truncation(name, cplx, seed, start):
    """``fixed`` with M at the largest bond, ``ret_s=True``, in both directions: the dense state to EPS, isometries, the
    bond dimensions of the oracle, and every row of the returned array the dense Schmidt spectrum of its bond,
    zero-padded and descending.
    Observed on MI355X: worst ratio 0.60 (isometries 5.97e-14 and dense state 4.51e-14 behind the complex 192 x 72
    block of the chain without a symmetry, whose small singular values cost the one-sided Jacobi columns their
    orthogonality first); 0.26 with the Holstein bond of 96, at most 0.15 on the bonds up to 40."""
    can = R.canonical(R.fixture(name, seed, cplx), start)
    psi, n = R.dense(can), can.nsite
    m = max(can.bond_dims)
    ref = can.copy()
    _, s_ref = orc.compress(ref, "fixed", max_dims=[m] * (n + 1))
    mps = R.to_device(_model(name), can)
    mps.compress_config = _fixed(m)
    out, rows = mps.compress(ret_s=True)
    assert out is mps and rows.shape[0] == n - 1
    _same_bookkeeping(mps, ref, exact=False)
    fig = _Figures(f"compress, nothing cut, {name} cplx={cplx} {start}")
    arrays = mps.to_arrays()
    assert all(a.dtype == np.dtype(complex if cplx else float) for a in arrays)
    fig.add("dense", R.rel(mps.todense(), psi), EPS)
    fig.add("isometries", R.isometry_error(arrays, mps.qnidx), EPS)
    _same_spectra(fig, rows, s_ref)
    bonds = range(1, n) if start == "right" else range(n - 1, 0, -1)
    for k, (bond, row) in enumerate(zip(bonds, rows), 1):
        dense_s = R.schmidt_values(psi, bond)
        w = min(len(row), len(dense_s))
        fig.add(f"sigma against the dense state, bond {bond}", np.abs(row[:w] - dense_s[:w]).max(), k * EPS * dense_s[0])
        rest = np.concatenate([row[w:], dense_s[w:], [0.0]])
        fig.add(f"sigma beyond the common width, bond {bond}", rest.max(), k * EPS * dense_s[0])
    fig.done()


@pytest.mark.parametrize("start", ("right", "left"))
@pytest.mark.parametrize("criteria", ("fixed", "threshold", "both"))
@pytest.mark.parametrize("name, cplx, seed", _pairs(R.TRUNC_CASES))
def test_compress_with_truncation(name, cplx, seed, criteria, start):
    """A ``criteria`` sweep (threshold 2e-2, M = 10) from the ``start`` side and a ``fixed`` sweep to M = 5 back - the
    second one runs system "R", sigma into the left factor and ``max_dims[idx]`` when the first went right, and the
    other branches when it went left.  After each: bond dimensions equal to the oracle's, singular values at
    every bond, labels as sorted multisets, the dense state against the oracle's.
    Observed on MI355X: worst ratio 0.023 over the 24 cases, always a singular value (3.2e-10 against 1.4e-8 at
    s[0] = 3.5e4); the dense states stay further below their bounds."""
    ref = R.truncation_reference(R.fixture(name, seed, cplx), criteria, start)
    g1, g2 = R.assert_conditions(ref)
    n = ref.canon.nsite
    mps = R.to_device(_model(name), ref.canon)
    fig = _Figures(f"compress {criteria} {name} cplx={cplx} {start}")
    mps.compress_config = CompressConfig(criteria, threshold=R.THR, max_bonddim=R.M1)
    _, rows = mps.compress(ret_s=True)
    _same_bookkeeping(mps, ref.first, exact=False)
    _same_spectra(fig, rows, ref.s1)
    fig.add("dense after the first sweep", R.rel(mps.todense(), R.dense(ref.first)), len(ref.gaps1) * EPS / g1)
    mps.compress_config = _fixed(R.M2)
    _, rows = mps.compress(ret_s=True)
    _same_bookkeeping(mps, ref.second, exact=False)
    _same_spectra(fig, rows, ref.s2, k0=n - 1)
    fig.add("dense after the second sweep", R.rel(mps.todense(), R.dense(ref.second)),
            (len(ref.gaps1) + len(ref.gaps2)) * EPS / min(g1, g2))
    assert mps.dtype == np.dtype(complex if cplx else float)
    fig.done()


@pytest.mark.parametrize("start", ("right", "left"))
@pytest.mark.parametrize("name, cplx, seed", _pairs(R.EY_CASES))
def test_one_bond_truncation_is_eckart_young(name, cplx, seed, start):
    """``temp_m_trunc`` as a list with inf everywhere but one bond - an inner one, the first, the last - on a sweep in
    either direction: the result is the dense SVD of the input cut at that bond (no oracle sweep involved; a list read
    one bond off cuts another bond).  Bound EPS / gap, the gap from the dense spectrum.
    Observed on MI355X: worst ratio 0.12 (1.50e-14 against 1.23e-13, the first bond cut to one value)."""
    can = R.canonical(R.fixture(name, seed, cplx), start)
    psi = R.dense(can)
    fig = _Figures(f"one-bond truncation {name} cplx={cplx} {start}")
    for bond, m in R.EY_BONDS:
        s = R.schmidt_values(psi, bond)
        gap = (s[m - 1] - s[m]) / s[0]
        assert gap >= R.MIN_GAP
        trunc = [np.inf] * (can.nsite + 1)
        trunc[bond] = m
        mps = R.to_device(_model(name), can)
        mps.compress(temp_m_trunc=trunc)
        assert mps.bond_dims[bond] == m and mps.to_right == (start != "right")
        fig.add(f"bond {bond} to {m}", R.rel(mps.todense(), R.best_rank_at_bond(psi, bond, m)), EPS / gap)
    fig.done()


@pytest.mark.parametrize("name, cplx, seeds", [(c[0], cplx, c[1 + cplx]) for c in R.SUM_CASES for cplx in (False, True)])
def test_rank_deficient_sums(name, cplx, seeds):
    """a + a through ``Mps.add``: after canonicalise, ``threshold=1e-8`` and, separately, ``fixed`` at the known rank
    bring the bond dimensions back to those of the canonicalised a, the state is 2 a, the values dropped are below
    1e-13 s[0] and those kept are twice the dense Schmidt values of a.  Then a.add(b) with prefactors that differ and
    ``compressed_sum([a, b, c], batchsize=2)`` without truncation against the dense sums.
    Observed on MI355X: worst ratio 0.45 (``compressed_sum``, four sweeps: 4.47e-14 against 1e-13); a + a and a.add(b)
    stay below 0.1."""
    model = _model(name)
    a, b, c = (R.fixture(name, s, cplx) for s in seeds)
    psi = R.dense(a)
    dims = R.canonical(a, "right").bond_dims
    n = a.nsite
    # the conditions, on the oracle's values
    ref = R.canonical(R.direct_sum(a, a), "right")
    _, s_ref = orc.compress(ref, "threshold", 1e-8)
    gaps = R.cut_gaps(s_ref, R.kept_dims(ref, True))
    assert ref.bond_dims == dims and gaps and min(gaps) >= R.MIN_GAP
    assert R.threshold_margin(s_ref, 1e-8) >= R.MIN_MARGIN
    fig = _Figures(f"sums {name} cplx={cplx}")
    twice = R.to_device(model, a).add(R.to_device(model, a))
    assert twice.bond_dims[1:-1] == [2 * d for d in a.bond_dims[1:-1]]
    fig.add("a + a", R.rel(twice.todense(), 2 * psi), EPS)
    twice.canonicalise()
    assert twice.bond_dims != dims
    fig.add("a + a canonicalised", R.rel(twice.todense(), 2 * psi), EPS)
    for cfg in (CompressConfig("threshold", threshold=1e-8), _fixed(max(dims), dims)):
        t = twice.copy()
        t.compress_config = cfg
        _, rows = t.compress(ret_s=True)
        _same_bookkeeping(t, ref, exact=False)
        assert t.bond_dims == dims
        fig.add(f"a + a compressed ({cfg.criteria.name})", R.rel(t.todense(), 2 * psi), len(gaps) * EPS / min(gaps))
        _same_spectra(fig, rows, s_ref)
        for k, (row, m) in enumerate(zip(rows, dims[1:-1]), 1):
            fig.add(f"values dropped at bond {k}", np.concatenate([row[m:], [0.0]]).max(), EPS * row[0])
            fig.add(f"values kept at bond {k}", np.abs(row[:m] - 2 * R.schmidt_values(psi, k)[:m]).max(),
                    k * EPS * row[0])
    # prefactors that differ are folded into the states
    a.coeff, b.coeff = (0.5j if cplx else 0.5), 2.0
    total = R.dense(a) + R.dense(b)
    both = R.to_device(model, a).add(R.to_device(model, b))
    assert both.dtype == np.dtype(complex if cplx else float)
    fig.add("a.add(b)", R.rel(both.todense(), total), EPS)
    both.canonicalise().compress(temp_m_trunc=np.inf)
    ref2 = R.canonical(R.direct_sum(a, b), "right")
    orc.compress(ref2, "fixed", max_dims=[10 ** 6] * (n + 1))
    _same_bookkeeping(both, ref2, exact=False)
    fig.add("a.add(b) compressed", R.rel(both.todense(), total), EPS)
    total = total + R.dense(c)
    three = compressed_sum([R.to_device(model, x) for x in (a, b, c)], batchsize=2, temp_m_trunc=np.inf)
    ref3 = R.canonical(R.direct_sum(c, ref2), "right")          # the queue of compressed_sum: c + the compressed a + b
    orc.compress(ref3, "fixed", max_dims=[10 ** 6] * (n + 1))
    _same_bookkeeping(three, ref3, exact=False)
    fig.add("compressed_sum", R.rel(three.todense(), total), EPS)
    fig.done()


@pytest.mark.parametrize("cplx", (False, True))
@pytest.mark.parametrize("name, op, seed_r, seed_c", R.OP_CASES)
def test_mpo_contract_svd(name, op, seed_r, seed_c, cplx):
    """``Mpo.contract(mps, algo="svd")`` with the Holstein Hamiltonian (labels -1, 0, 1 on its bonds: up to four label
    groups and blocks that are exactly zero in one decomposition) and with the creation operator, which shifts the total
    charge.  The product: bonds multiply, labels add - against the host twin of ``Mpo.apply``.  The sweeps: the oracle's on
    the product read back from the device, cut to M = 10.
    Observed on MI355X: worst ratio 0.013 (the canonicalised product, 1.27e-15)."""
    model = _model(name)
    st = R.fixture(name, seed_c if cplx else seed_r, cplx)
    mpo = Mpo(model) if op == "H" else Mpo.onsite(model, r"a^\dagger")
    mps = R.to_device(model, st)
    mps.compress_config = _fixed(R.OP_M)
    fig = _Figures(f"contract {op} {name} cplx={cplx}")
    prod_dev = mpo.apply(mps)
    prod = R.to_oracle(prod_dev)
    twin = R.operator_reference(mpo, st)[0]
    assert prod.bond_dims == [x * y for x, y in zip(st.bond_dims, mpo.bond_dims)]
    assert prod.qntot[0] == st.qntot[0] + (op != "H")
    _same_bookkeeping(prod_dev, twin, exact=True)
    fig.add("product", R.rel(R.dense(prod), R.dense(twin)), EPS)
    canon, out, s_ref, gaps = R.fixed_reference(prod, R.OP_M)
    assert gaps and min(gaps) >= R.MIN_GAP
    bound = len(gaps) * EPS / min(gaps)
    # the steps of contract, with the singular values
    prod_dev.canonicalise()
    _same_bookkeeping(prod_dev, canon, exact=True)
    fig.add("product canonicalised", R.rel(prod_dev.todense(), R.dense(prod)), EPS)
    _, rows = prod_dev.compress(ret_s=True)
    _same_bookkeeping(prod_dev, out, exact=False)
    _same_spectra(fig, rows, s_ref)
    fig.add("product compressed", R.rel(prod_dev.todense(), R.dense(out)), bound)
    res = mpo.contract(mps, algo="svd")
    _same_bookkeeping(res, out, exact=False)
    assert max(res.bond_dims) == R.OP_M and res.dtype == np.dtype(complex if cplx else float)
    fig.add("contract", R.rel(res.todense(), R.dense(out)), bound)
    fig.done()


@pytest.mark.parametrize("cplx", (False, True))
def test_mpdm_canonicalise_and_compress(cplx):
    """``MpDm.from_mps``, ``mpo.apply(rho)``, ``canonicalise``, ``compress`` against the oracle on the folded sites
    (D_l, d * d, D_r) with the labels add_outer(up, 0); the dense operator from ``MpDm.todense()``.  Two molecules: the
    dense operator of three has 1.9e8 entries.
    Observed on MI355X: worst ratio 0.033 (a singular value of the second bond, 4.7e-14 against 1.4e-12)."""
    name, *seeds = R.MPDM_CASE
    model = _model(name)
    ds = list(model.pbond_list)
    st = R.fixture(name, seeds[cplx], cplx)
    mpo = Mpo(model)
    fig = _Figures(f"density operator cplx={cplx}")
    rho = MpDm.from_mps(R.to_device(model, st))
    fig.add("from_mps", R.rel(rho.todense(), np.diag(R.dense(st).ravel())), EPS)
    prod_dev = mpo.apply(rho)
    assert isinstance(prod_dev, MpDm) and prod_dev[0].ndim == 4
    prod = R.to_oracle(prod_dev)
    twin = R.operator_reference(mpo, R.diagonal_operator(st))[0]
    _same_bookkeeping(prod_dev, twin, exact=True)
    fig.add("product", R.rel(R.dense(prod), R.dense(twin)), EPS)
    fig.add("product, todense", R.rel(R.fold_dense_operator(prod_dev.todense(), ds), R.dense(twin)), EPS)
    canon, out, s_ref, gaps = R.fixed_reference(prod, R.OP_M)
    assert gaps and min(gaps) >= R.MIN_GAP
    prod_dev.canonicalise()
    _same_bookkeeping(prod_dev, canon, exact=True)
    arrays = [a.reshape(a.shape[0], -1, a.shape[-1]) for a in prod_dev.to_arrays()]
    fig.add("canonicalised", R.rel(R.fold_dense_operator(prod_dev.todense(), ds), R.dense(prod)), EPS)
    fig.add("isometries", R.isometry_error(arrays, 0), EPS)
    prod_dev.compress_config = _fixed(R.OP_M)
    _, rows = prod_dev.compress(ret_s=True)
    _same_bookkeeping(prod_dev, out, exact=False)
    _same_spectra(fig, rows, s_ref)
    assert prod_dev[1].ndim == 4 and max(prod_dev.bond_dims) == R.OP_M
    fig.add("compressed", R.rel(R.fold_dense_operator(prod_dev.todense(), ds), R.dense(out)),
            len(gaps) * EPS / min(gaps))
    fig.done()
