"""Quantum-number chains, dense references and sweep conditions for the canonicalise / compress sweeps, shared by
tests/test_compress_refs_host.py and tests/test_compress_gpu.py.  Host only: NumPy and the oracle, no engine (``to_device``
and ``holstein_model`` import the package when they are called).

Conventions: sites are arrays (D_l, d, D_r); bond k lies left of site k, so the inner bonds are 1 .. n - 1 and a state
of n sites has n + 1 label lists.  A chain is described by the labels of its bonds counted from the LEFT (charge
accumulated up to the bond), the last one being the total charge.  The chains are those of the 9-site Holstein model of
tests/test_observables_gpu.py - three molecules of an electronic two-level site and two vibrations (d = 2, 4, 3; one
conserved charge carried by the electronic sites) - and the same physical legs without a symmetry (every label zero: one
block per decomposition).

With one charge in three electronic sites a decomposition of the Holstein chain has at most two blocks that find a
partner, so the block kinds the kernels treat differently are spread over the decompositions of ONE sweep of the
``ragged`` fixture (``sweep_blocks`` lists them, the host test pins them): after the canonicalisation the right-going SVD
meets a 1 x 1 block next to a 12 x 19 one (wider than tall: the adjoint path) and 11 rows whose label has no partner
column at the second electronic site, a single-column 9 x 1 block at the site before it and a 48 x 21 block after it."""
from types import SimpleNamespace

import numpy as np

from oracle import mps_oracle as orc

HOLSTEIN_D = (2, 4, 3)


def holstein_sigmaqn(nmol=3):
    """(d, 1) labels per site of ``nmol`` molecules: the electronic site carries 0 / 1, the vibrations nothing"""
    return [np.array([[0], [1]]), np.zeros((4, 1), dtype=int), np.zeros((3, 1), dtype=int)] * nmol


def nosym_sigmaqn(nmol=3):
    return [np.zeros((d, 1), dtype=int) for d in HOLSTEIN_D * nmol]


def chain_model(sigmaqn):
    """What ``Mps`` reads of a model for the sweeps and ``todense``: for chains that no Hamiltonian goes with"""
    return SimpleNamespace(basis=[SimpleNamespace(sigmaqn=np.asarray(s), nbas=len(s)) for s in sigmaqn],
                           pbond_list=[len(s) for s in sigmaqn], nsite=len(sigmaqn), qn_size=np.asarray(sigmaqn[0]).shape[-1])


def labels(n0, n1):
    """n0 zeros and n1 ones, the ones spread evenly: the rows of a block are not contiguous"""
    n = n0 + n1
    return [((i + 1) * n1) // n - (i * n1) // n for i in range(n)]


def _bonds01(pairs, qntot=1):
    return [[0]] + [labels(*p) for p in pairs] + [[qntot]]


# name -> (sigmaqn, labels of the bonds 0 .. n counted from the left, decay).  Bonds stay at 40 or below except in the
# two ``wide`` chains (complex only), whose bond 5 of 96 gives the QR a 96-row block and leaves the SVD blocks of 72 and
# 36 columns.  ``ragged`` has bonds wider than the rank the chain can carry (bonds 4 and 5), as a sum of states has.
FIXTURES = {
    "ragged": (holstein_sigmaqn(), _bonds01([(1, 1), (3, 4), (1, 11), (1, 19), (1, 30), (5, 9), (0, 7), (0, 3)]), None),
    "holstein": (holstein_sigmaqn(), _bonds01([(1, 1), (4, 4), (8, 12), (10, 20), (12, 28), (12, 12), (0, 12), (0, 3)]),
                 0.9),
    "holstein_wide": (holstein_sigmaqn(), _bonds01([(1, 1), (4, 4), (12, 12), (12, 24), (26, 70), (12, 12), (0, 12),
                                                    (0, 3)]), None),
    "nosym": (nosym_sigmaqn(), [[0] * b for b in (1, 2, 7, 13, 20, 17, 11, 6, 3, 1)], 0.85),
    "nosym_wide": (nosym_sigmaqn(), [[0] * b for b in (1, 2, 8, 24, 48, 96, 24, 12, 3, 1)], None),
    # bonds of 13 and 8: sums of three states and products with the Holstein operator (bonds up to 5) stay at 40
    "holstein_small": (holstein_sigmaqn(), _bonds01([(1, 1), (3, 4), (4, 6), (4, 9), (4, 9), (4, 8), (0, 7), (0, 3)]),
                       None),
    "nosym_small": (nosym_sigmaqn(), [[0] * b for b in (1, 2, 6, 9, 13, 11, 8, 5, 3, 1)], None),
    "holstein_tiny": (holstein_sigmaqn(), _bonds01([(1, 1), (2, 3), (3, 5), (3, 5), (3, 5), (3, 4), (0, 4), (0, 3)]),
                      None),
    # no charge: what the creation operator is applied to
    "holstein_q0": (holstein_sigmaqn(), [[0] * b for b in (1, 1, 4, 8, 8, 8, 8, 8, 3, 1)], None),
    # two molecules: the chain of the density-operator test (the dense operator of three has 1.9e8 entries)
    "holstein6": (holstein_sigmaqn(2), _bonds01([(1, 1), (3, 3), (3, 5), (0, 6), (0, 3)]), None),
}
COMPLEX_ONLY = ("holstein_wide", "nosym_wide")

# (fixture, seed for the real chain, seed for the complex one) of every comparison of tests/test_compress_gpu.py; the
# seeds are those tests/test_compress_refs_host.py finds the gap and margin conditions met for
EXACT_CASES = (("ragged", 1, 2), ("nosym", 1, 2), ("holstein_wide", None, 3), ("nosym_wide", None, 4))
TRUNC_CASES = (("holstein", 3, 4), ("nosym", 1, 6))
M1, M2, THR = 10, 5, 2e-2            # first sweep, second (fixed) sweep, threshold of the first
EY_CASES = TRUNC_CASES
EY_BONDS = ((4, 7), (1, 1), (8, 2))  # (bond, values kept): an inner bond, the first and the last
SUM_CASES = (("holstein_small", (16, 17, 15), (15, 17, 18)), ("nosym_small", (11, 12, 13), (14, 15, 16)))
OP_CASES = (("holstein_tiny", "H", 29, 27), ("holstein_q0", "a^dagger", 21, 25))     # (fixture, operator, seeds)
MPDM_CASE = ("holstein6", 22, 22)
OP_M = 10                        # bond dimension the products with an operator are cut to
MIN_GAP = MIN_MARGIN = 1e-3


def fixture(name, seed, cplx):
    sigmaqn, bond_qn, decay = FIXTURES[name]
    return random_qn_chain(np.random.default_rng(seed), sigmaqn, bond_qn, cplx, decay)


def random_qn_chain(rng, sigmaqn, bond_qn, cplx, decay=None):
    """``orc.MpsState`` with site tensors (D_l, d, D_r): standard normal where label_l + sigma == label_r, exactly zero
    elsewhere; per site the real part is drawn first, then the imaginary part.  ``decay``: column r of every site is
    multiplied by decay ** r, which gives the bonds decaying Schmidt spectra.  The state has the convention of
    ``Mps.random``: qnidx = nsite - 1, to_right = False, so the last label list (the total charge, counted from the
    left) is stored counted from the right: zero."""
    n = len(sigmaqn)
    assert len(bond_qn) == n + 1
    q = np.asarray(sigmaqn[0]).shape[-1]
    qn = [np.asarray(b, dtype=int).reshape(-1, q) for b in bond_qn]
    assert len(qn[0]) == 1 and len(qn[-1]) == 1
    qntot = qn[-1][0].copy()
    sites = []
    for i in range(n):
        sig = np.asarray(sigmaqn[i], dtype=int).reshape(-1, q)
        shape = (len(qn[i]), len(sig), len(qn[i + 1]))
        a = rng.standard_normal(shape)
        if cplx:
            a = a + 1j * rng.standard_normal(shape)
        mask = np.all(qn[i][:, None, None, :] + sig[None, :, None, :] == qn[i + 1][None, None, :, :], axis=-1)
        a[~mask] = 0
        if decay is not None:
            a = a * decay ** np.arange(shape[2])
        sites.append(a)
    qn[-1] = qntot - qn[-1]
    return orc.MpsState(sites, qn, n - 1, qntot, False, [np.asarray(s, dtype=int).reshape(-1, q) for s in sigmaqn])


def dense(state):
    """the wavefunction, one axis per site"""
    t = state.sites[0].reshape(-1, state.sites[0].shape[-1])
    for a in state.sites[1:]:
        t = (t @ a.reshape(a.shape[0], -1)).reshape(-1, a.shape[-1])
    return t.reshape([a.shape[1] for a in state.sites]) * state.coeff


def direct_sum(a, b):
    """The oracle-side twin of ``Mps.add``: block-diagonal sites, label lists concatenated.  Prefactors that differ are
    folded into the centre sites first."""
    assert a.nsite == b.nsite and a.nsite > 1 and a.qnidx == b.qnidx and a.to_right == b.to_right
    assert np.array_equal(a.qntot, b.qntot)
    a, b = a.copy(), b.copy()
    if not np.allclose(a.coeff, b.coeff):
        for st in (a, b):
            st.sites[st.qnidx] = st.sites[st.qnidx] * st.coeff
            st.coeff = 1.0
    n, sites = a.nsite, []
    for i, (x, y) in enumerate(zip(a.sites, b.sites)):
        la, ra, lb, rb = x.shape[0], x.shape[-1], y.shape[0], y.shape[-1]
        if i == 0:
            out = np.concatenate([x, y], axis=-1)
        elif i == n - 1:
            out = np.concatenate([x, y], axis=0)
        else:
            out = np.zeros((la + lb,) + x.shape[1:-1] + (ra + rb,), dtype=np.result_type(x, y))
            out[:la, ..., :ra] = x
            out[la:, ..., ra:] = y
        sites.append(out)
    qn = [a.qn[0].copy()] + [np.concatenate([p, r]) for p, r in zip(a.qn[1:-1], b.qn[1:-1])] + [a.qn[-1].copy()]
    return orc.MpsState(sites, qn, a.qnidx, a.qntot.copy(), a.to_right, a.sigmaqn, a.coeff)


def apply_mpo(mpo_sites, mpo_qn, mpo_qntot, state):
    """The oracle-side twin of ``Mpo.apply`` for an operator whose labels are counted like the state's (both centred
    on the last site): site = einsum("apqb,cqd->acpbd"), labels added, the total shifted."""
    assert state.qnidx == state.nsite - 1 and not state.to_right
    sites = []
    for w, a in zip(mpo_sites, state.sites):
        if a.ndim == 4:             # density-operator site: the operator meets the upper leg
            t = np.einsum("apqb,cqrd->acprbd", w, a)
            sites.append(t.reshape(w.shape[0] * a.shape[0], w.shape[1], a.shape[2], w.shape[3] * a.shape[3]))
            continue
        t = np.einsum("apqb,cqd->acpbd", w, a)
        sites.append(t.reshape(w.shape[0] * a.shape[0], w.shape[1], w.shape[3] * a.shape[2]))
    qn = [orc.add_outer(np.asarray(qo), np.asarray(qs)).reshape(-1, len(state.qntot)) for qo, qs in zip(mpo_qn, state.qn)]
    return orc.MpsState(sites, qn, state.qnidx, state.qntot + np.asarray(mpo_qntot), False, state.sigmaqn, state.coeff)


def fold_mpdm(sites, sigmaqn):
    """density-operator sites (D_l, d, d, D_r) as MPS sites (D_l, d * d, D_r) with the labels add_outer(up, 0) of the
    leg pair - only the upper leg carries charge: the oracle's sweeps then serve ``MpDm`` too"""
    out, sig = [], []
    for a, s in zip(sites, sigmaqn):
        a = np.asarray(a)
        assert a.ndim == 4 and a.shape[1] == a.shape[2] == len(s)
        out.append(a.reshape(a.shape[0], -1, a.shape[-1]))
        up = np.asarray(s)
        sig.append(orc.add_outer(up, np.zeros_like(up)).reshape(-1, up.shape[-1]))
    return out, sig


def diagonal_operator(state):
    """The oracle-side twin of ``MpDm.from_mps``: sites (D_l, d, d, D_r) with the amplitudes on the diagonal of the leg
    pair.  The state keeps the labels (d, q) of the upper leg: ``folded`` is what the sweeps take."""
    sites = []
    for a in state.sites:
        mo = np.zeros((a.shape[0], a.shape[1], a.shape[1], a.shape[2]), dtype=a.dtype)
        for k in range(a.shape[1]):
            mo[:, k, k, :] = a[:, k, :]
        sites.append(mo)
    new = state.copy()
    new.sites = sites
    return new


def folded(state):
    """a state of density-operator sites with ``fold_mpdm`` applied to its sites and labels"""
    new = state.copy()
    new.sites, new.sigmaqn = fold_mpdm(state.sites, state.sigmaqn)
    return new


def fold_dense_operator(mat, ds):
    """the (prod d) x (prod d) matrix of ``MpDm.todense`` with one axis of d * d per site, as ``dense`` of the folded
    chain has them"""
    n = len(ds)
    t = np.asarray(mat).reshape(tuple(ds) + tuple(ds))
    t = t.transpose([k for i in range(n) for k in (i, n + i)])
    return t.reshape([d * d for d in ds])


def rel(x, y):
    """|x - y| / |y|, 2-norms"""
    return float(np.linalg.norm(np.asarray(x) - np.asarray(y)) / np.linalg.norm(y))


def isometry_error(sites, centre):
    """largest entry of |A^H A - 1| over the sites left of ``centre`` and of |A A^H - 1| over those right of it"""
    worst = 0.0
    for i, a in enumerate(sites):
        if i == centre:
            continue
        m = a.reshape(-1, a.shape[-1]) if i < centre else a.reshape(a.shape[0], -1).conj().T
        worst = max(worst, float(np.abs(m.conj().T @ m - np.eye(m.shape[1])).max()))
    return worst


def _bipartition(psi, bond):
    psi = np.asarray(psi)
    assert 1 <= bond <= psi.ndim - 1
    return psi.reshape(int(np.prod(psi.shape[:bond])), -1)


def schmidt_values(psi, bond):
    """singular values, descending, of the dense state cut at ``bond``"""
    return np.linalg.svd(_bipartition(psi, bond), compute_uv=False)


def best_rank_at_bond(psi, bond, m):
    """the closest state of Schmidt rank m at ``bond`` (Eckart-Young): the dense SVD of the bipartition, truncated"""
    u, s, vh = np.linalg.svd(_bipartition(psi, bond), full_matrices=False)
    return ((u[:, :m] * s[:m]) @ vh[:m]).reshape(np.shape(psi))


def cut_gaps(s_list, dims):
    """(s[m - 1] - s[m]) / s[0] for every decomposition of a sweep that kept m = dims[i] of more values"""
    return [float((s[m - 1] - s[m]) / s[0]) for s, m in zip(s_list, dims) if m < len(s)]


def threshold_margin(s_list, thr):
    """min |s / |s| - thr| / thr over all values of a sweep: how far the threshold count is from a tie"""
    return min(float(np.min(np.abs(np.asarray(s) / np.linalg.norm(s) - thr))) for s in s_list) / thr


def kept_dims(state_after, to_right):
    """the bond dimensions a finished sweep left behind, in the order of its decompositions"""
    inner = state_after.bond_dims[1:-1]
    return inner if to_right else inner[::-1]


def sweep_blocks(state, sweep):
    """[(site, [(rows, columns) of every block], rows without a partner)] of the decompositions of ``sweep(state)``;
    the state is changed as the sweep changes it"""
    rec, orig = [], orc.qn_blocks

    def spy(qnbigl, qnbigr, qntot):
        blocks = orig(qnbigl, qnbigr, qntot)
        nrow = int(np.prod(np.asarray(qnbigl).shape[:-1]))
        rec.append(([(len(b[2]), len(b[3])) for b in blocks], nrow - sum(len(b[2]) for b in blocks)))
        return blocks

    sites = list(state.iter_idx_list(full=False))
    orc.qn_blocks = spy
    try:
        sweep(state)
    finally:
        orc.qn_blocks = orig
    assert len(rec) == len(sites)
    return [(i,) + r for i, r in zip(sites, rec)]


def canonical(state, start):
    """a copy canonicalised by the oracle so that the next sweep goes right from site 0 (start == "right": one sweep
    from the convention of ``random_qn_chain``) or left from the last site (start == "left": a second sweep)"""
    st = state.copy()
    orc.canonicalise(st)
    if start == "left":
        orc.canonicalise(st)
    assert st.to_right == (start == "right") and st.qnidx == (0 if st.to_right else st.nsite - 1)
    return st


def truncation_reference(state, criteria, start, m1=M1, m2=M2, thr=THR):
    """The oracle's ``criteria`` sweep (threshold thr, at most m1 values) from the ``start`` side and the tighter fixed
    sweep (m2) back, on the canonicalised ``state``.  canon / first / second: the state before, between and after;
    s1 / s2: the singular values per decomposition; gaps1 / gaps2: ``cut_gaps``; margin: ``threshold_margin`` of the
    first sweep (None for "fixed")."""
    canon = canonical(state, start)
    n = canon.nsite
    first = canon.copy()
    _, s1 = orc.compress(first, criteria, thr, [m1] * (n + 1))
    second = first.copy()
    _, s2 = orc.compress(second, "fixed", max_dims=[m2] * (n + 1))
    right = start == "right"
    return SimpleNamespace(canon=canon, first=first, second=second, s1=s1, s2=s2,
                           gaps1=cut_gaps(s1, kept_dims(first, right)), gaps2=cut_gaps(s2, kept_dims(second, not right)),
                           margin=None if criteria == "fixed" else threshold_margin(s1, thr))


def assert_conditions(ref):
    """What keeps a comparison of truncated states from being decided by a near-tie: both sweeps cut, every cut has a
    gap of MIN_GAP, the threshold count a margin of MIN_MARGIN.  Returns the smallest gap per sweep."""
    assert ref.gaps1 and ref.gaps2, (ref.gaps1, ref.gaps2)
    assert min(ref.gaps1) >= MIN_GAP and min(ref.gaps2) >= MIN_GAP, (ref.gaps1, ref.gaps2)
    assert ref.margin is None or ref.margin >= MIN_MARGIN, ref.margin
    return min(ref.gaps1), min(ref.gaps2)


def fixed_reference(state, m):
    """canonicalise and one fixed sweep to ``m`` by the oracle, as ``Mpo.contract(algo="svd")`` does to its product:
    (canonicalised state, compressed state, singular values, cut gaps)"""
    canon = canonical(state, "right")
    out = canon.copy()
    _, s = orc.compress(out, "fixed", max_dims=[m] * (canon.nsite + 1))
    return canon, out, s, cut_gaps(s, kept_dims(out, True))


def holstein_model(nmol=3):
    """the Holstein model of tests/test_observables_gpu.py with ``nmol`` molecules (host-side model layer)"""
    from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity
    ph = [Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.274571056529368), 4),
          Phonon.simple_phonon(Quantity(3.1e-3), Quantity(9.5), 3)]
    return HolsteinModel([Mol(Quantity(0), ph)] * nmol, Quantity(3.0e-2), 3)


def operator_reference(mpo, state, m=OP_M):
    """``Mpo.contract(state, algo="svd")`` restated: (product, canonicalised, compressed, singular values, cut gaps);
    a state of density-operator sites is folded after the product"""
    prod = apply_mpo([mpo[i] for i in range(len(mpo))], mpo.qn, mpo.qntot, state)
    if prod.sites[0].ndim == 4:
        prod = folded(prod)
    return (prod,) + fixed_reference(prod, m)


def to_oracle(mps):
    """the device state read back; a density operator comes folded"""
    sites = mps.to_arrays()
    q = len(mps.qntot)
    sig = [np.asarray(b.sigmaqn).reshape(-1, q) for b in mps.model.basis]
    if sites[0].ndim == 4:
        sites, sig = fold_mpdm(sites, sig)
    return orc.MpsState(sites, [np.array(x).reshape(-1, q) for x in mps.qn], mps.qnidx, np.array(mps.qntot), mps.to_right,
                        sig, mps.coeff)


def to_device(model, state, cls=None):
    """``state`` uploaded through ``cls.from_arrays`` (cls: ``Mps``, the default, or a subclass)"""
    if cls is None:
        from renormalizer_amd.mps.mps import Mps as cls
    return cls.from_arrays(model, state.sites, [x.copy() for x in state.qn], state.qnidx, state.qntot.copy(),
                           state.to_right, state.coeff)
