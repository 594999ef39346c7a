"""GPU parity of the DMRG path (optimize_mps: environments, Heff matvec, Davidson, full block SVD + basis
selection) against the reference's own known answers.  pytest -m gpu."""
import os

import numpy as np
import pytest

from renormalizer_amd import HolsteinModel, Model, Mol, Mpo, Phonon, Quantity
from renormalizer_amd.model import h_qc
from renormalizer_amd.utils import constant

pytestmark = pytest.mark.gpu


def _holstein_test_model():
    """renormalizer/tests/parameter.py:7-34 (3 molecules x 2 modes, 4 phonon levels)."""
    omega = [Quantity(106.51, "cm^{-1}"), Quantity(1555.55, "cm^{-1}")]
    dis = [Quantity(30.1370), Quantity(8.7729)]
    ph_list = [Phonon.simple_phonon(o, d, 4) for o, d in zip(omega, dis)]
    j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
    return HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list, 15.45)] * 3, j, 3)


@pytest.mark.parametrize("method", ["2site", "1site"])
def test_holstein_ground_state(method):
    """mps/tests/test_gs.py:21-37: E_gs = 0.08401412 + ZPE (rel 1e-5) and <H> of the returned state."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    model = _holstein_test_model()
    mpo = Mpo(model)
    gs_e = 0.08401412 + model.gs_zpe
    procedure = [[10, 0.4], [20, 0.2], [30, 0.1], [40, 0], [40, 0]]
    mps = Mps.random(model, 1, procedure[0][0], rng=np.random.default_rng(2019))
    mps.optimize_config.procedure = procedure
    mps.optimize_config.method = method
    energies, opt = optimize_mps(mps.copy(), mpo)
    assert energies[-1] == pytest.approx(gs_e, rel=1e-5)
    assert opt.expectation(mpo) == pytest.approx(gs_e, rel=1e-5)
    assert abs(opt.mp_norm - 1.0) < 1e-10
    # 1-site sweep energies of the reference for this model converge to the same value
    assert min(energies) == pytest.approx(0.0953734687866298, abs=2e-7)


def test_h2o_dmrg_with_fermionic_on_the_fly_swapping(golden_dir):
    """mps/tests/test_gs.py:120-146 (test_qc with_ofs): two-site DMRG of a Jordan-Wigner chain with on-the-fly
    swapping of neighbouring spin orbitals, ``ofs_swap_jw=True``: the exchanged two-site tensor carries the fermionic
    sign (mps/mp.py:711-714) and the MPO follows through ``Mpo.try_swap_site(..., swap_jw=True)``.  The reference's
    bar is 5e-3 on the FCI energy at M = 30; here water / STO-3G.  <H> of the returned state in ITS orbital order, with
    an MPO built from scratch for that order, is the end-to-end check of the signs."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    from renormalizer_amd.utils import OFS, CompressConfig, CompressCriteria
    sh, aseri, nuc = h_qc.read_fcidump(os.path.join(golden_dir, "h2o_fcidump.txt"), 7)
    # a shuffled order of the spatial orbitals (both spin orbitals of an orbital move together, so the alpha / beta
    # labelling by position stays valid): the energy does not depend on it, the entanglement along the chain does,
    # and the sweeps have something to exchange
    sp = np.random.default_rng(5).permutation(7)
    so = np.array([2 * p + s for p in sp for s in (0, 1)])
    sh, aseri = sh[np.ix_(so, so)], aseri[np.ix_(so, so, so, so)]
    basis, terms = h_qc.qc_model(sh, aseri)
    model = Model(basis, terms)
    mpo = Mpo(model)
    M = 30
    mps = Mps.random(model, [5, 5], M, percent=1.0, rng=np.random.default_rng(1))
    # (the swapping options travel in the procedure: an integer entry makes optimize_mps build a plain
    # CompressConfig for that sweep, here as in the reference, gs.py:124-131)
    cc = CompressConfig(CompressCriteria.fixed, max_bonddim=M, ofs=OFS.ofs_s, ofs_swap_jw=True)
    mps.optimize_config.procedure = [[cc, 0.4], [cc, 0.2], [cc, 0.1], [cc, 0], [cc, 0], [cc, 0]]
    mps.optimize_config.method = "2site"
    swaps = []
    plain_swap = Mpo.try_swap_site

    def counting_swap(self, new_model, swap_jw=False, **kw):
        if any(b1.dofs != b2.dofs for b1, b2 in zip(self.model.basis, new_model.basis)):
            swaps.append(bool(swap_jw))
        return plain_swap(self, new_model, swap_jw, **kw)

    Mpo.try_swap_site = counting_swap
    try:
        energies, opt = optimize_mps(mps, mpo)
    finally:
        Mpo.try_swap_site = plain_swap
    fci = -75.008697516450 - nuc
    assert abs(min(energies) - fci) < 5e-3
    assert len(swaps) > 0 and all(swaps)                              # sites were exchanged, with the fermionic sign
    def energy_in_own_order(state):
        """<H> with an MPO built from scratch for the state's site order, without quantum numbers"""
        order = [b.dofs[0] for b in state.model.basis]
        assert sorted(order) == list(range(14))
        rebuilt = Mpo(Model(*h_qc.qc_model(sh[np.ix_(order, order)], aseri[np.ix_(order, order, order, order)],
                                           conserve_qn=False)))
        plain = Mps.from_arrays(rebuilt.model, state.to_arrays(),
                                [np.zeros((d, 1), dtype=int) for d in state.bond_dims], 0, np.array([0]), True)
        return plain.expectation(rebuilt)

    # the swept state and the swapped MPO end in the same site order, and the swapped MPO is the Hamiltonian of that
    # order: an operator rebuilt for it gives the same <H> (a missing sign on either side shows at the 0.1 level)
    assert [b.dofs for b in mps.model.basis] == [b.dofs for b in mpo.model.basis]
    assert [b.dofs[0] for b in mps.model.basis] != list(range(14))
    assert abs(energy_in_own_order(mps) - mps.expectation(mpo)) < 1e-8
    # the returned state is the copy taken at the previous sweep's optimal centre (gs.py:288-291); its site order is
    # the one of that moment, its energy the converged one
    assert abs(energy_in_own_order(opt) - fci) < 5e-3


@pytest.mark.parametrize("method", ["2site", "1site"])
def test_optimize_config_inverse(method):
    """``optimize_config.inverse = -1`` (utils/configs.py:292-294; gs.py:397-398, 470, 521): the centre problems are those
    of -H, i.e. the sweep climbs to the HIGHEST state of the sector, and the values returned are eigenvalues of the scaled
    operator.  Pinned three ways on a model small enough for a dense spectrum: (i) against DMRG of the negated MPO with
    inverse = +1 (the plain path), (ii) against the largest eigenvalue of the dense Hamiltonian restricted to the
    one-exciton sector, (iii) <H> of the returned state.  Both the dense centre solver (centres below 1000 elements) and
    the Davidson iteration (bond dimension 16 -> larger centres) are on the path."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    # four molecules x one mode x four levels: 4096 states in all, 1024 in the one-exciton sector; at M = 16 the centres
    # of the middle of the chain have 1024 (one-site) / 2048 (two-site) elements: Davidson; the outer ones are dense
    ph = [Phonon.simple_phonon(Quantity(1555.55, "cm^{-1}"), Quantity(8.7729), 4)]
    j = np.zeros((4, 4))
    for a in range(3):
        j[a, a + 1] = j[a + 1, a] = -0.1 * (a + 1) / constant.au2ev
    model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph, 15.45)] * 4, j, 3)
    mpo = Mpo(model)
    procedure = [[16, 0.4], [16, 0.2], [16, 0.1], [16, 0], [16, 0], [16, 0]]

    def run(op, inverse):
        mps = Mps.random(model, 1, 16, rng=np.random.default_rng(11))
        mps.optimize_config.procedure = procedure
        mps.optimize_config.method = method
        mps.optimize_config.inverse = inverse
        return optimize_mps(mps, op)

    e_inv, top = run(mpo, -1.0)
    e_neg, top2 = run(mpo.scale(-1.0), 1.0)
    assert min(e_inv) == pytest.approx(min(e_neg), abs=1e-8)
    # <H> of the state the inverse sweep returns: the highest level, so -<H> is the converged value
    assert -top.expectation(mpo) == pytest.approx(min(e_inv), abs=1e-7)
    assert abs(top.mp_norm - 1.0) < 1e-10
    # the plain sweep finds the other end of the spectrum
    e_gs, _ = run(mpo, 1.0)
    assert min(e_gs) < -min(e_inv) - 1e-3
    # dense spectrum of the one-exciton sector: electronic occupation numbers are diagonal in the product basis
    dense = mpo.todense()
    nex = np.zeros(dense.shape[0])
    dims = [int(d) for d in model.pbond_list]
    idx = np.indices(dims).reshape(len(dims), -1)
    for site, b in enumerate(model.basis):
        sq = np.asarray(b.sigmaqn).reshape(dims[site], -1)[:, 0]
        nex += sq[idx[site]]
    sector = nex == 1
    w = np.linalg.eigvalsh(dense[np.ix_(sector, sector)])
    assert -min(e_inv) == pytest.approx(w[-1], abs=1e-6)
    assert min(e_gs) == pytest.approx(w[0], abs=1e-6)


@pytest.mark.parametrize("nroots", [1, 3])
def test_primme_style_solver_option(nroots):
    """optimize_config.algo = "primme" (gs.py:552-569: the reference hands the centre problems to PRIMME with
    tol = 1e-6 on the residual and the diagonal preconditioner): here the engine's block Davidson with PRIMME's
    convergence test and restart space.  Same ground / state-averaged energies as algo = "davidson" to the solver
    tolerance; an unknown algo is refused like the reference's ``assert False``."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    model = _holstein_test_model()
    mpo = Mpo(model)
    procedure = [[10, 0.4], [20, 0.2], [30, 0.1], [40, 0], [40, 0]]
    out = {}
    for algo in ("davidson", "primme"):
        mps = Mps.random(model, 1, procedure[0][0], rng=np.random.default_rng(2019))
        mps.optimize_config.procedure = procedure
        mps.optimize_config.method = "2site"
        mps.optimize_config.nroots = nroots
        mps.optimize_config.algo = algo
        energies, _ = optimize_mps(mps, mpo)
        out[algo] = np.atleast_1d(np.asarray(energies[-1], dtype=float))
    assert out["primme"].shape == out["davidson"].shape
    assert np.abs(out["primme"] - out["davidson"]).max() < 1e-7
    if nroots == 1:
        assert out["primme"][0] == pytest.approx(0.08401412 + model.gs_zpe, rel=1e-5)
    mps = Mps.random(model, 1, 10, rng=np.random.default_rng(1))
    mps.optimize_config.procedure = procedure
    mps.optimize_config.algo = "arpack"
    with pytest.raises(ValueError):
        optimize_mps(mps, mpo)


def test_h2o_sto3g_fci_energy(golden_dir):
    """example/h2o_qc.py: water STO-3G (10e, 7o), 2-site DMRG at M = 50 reaches the FCI energy -75.008697516450."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    sh, aseri, nuc = h_qc.read_fcidump(os.path.join(golden_dir, "h2o_fcidump.txt"), 7)
    basis, terms = h_qc.qc_model(sh, aseri)
    model = Model(basis, terms)
    mpo = Mpo(model)
    assert mpo.bond_dims == [1, 4, 16, 33, 46, 71, 92, 77, 60, 69, 54, 33, 16, 4, 1]     # reference, algo "qr"
    M = 50
    mps = Mps.random(model, [5, 5], M, percent=1.0, rng=np.random.default_rng(1))
    mps.optimize_config.procedure = [[M, 0.4], [M, 0.2], [M, 0.1], [M, 0], [M, 0], [M, 0], [M, 0]]
    mps.optimize_config.method = "2site"
    energies, opt = optimize_mps(mps.copy(), mpo)
    gs_e = min(energies) + nuc
    assert abs(gs_e - (-75.008697516450)) < 1e-8
    assert abs(opt.expectation(mpo) + nuc - (-75.008697516450)) < 1e-7
    # particle numbers are conserved exactly by the block structure
    assert opt.qntot.tolist() == [5, 5]


@pytest.mark.parametrize("method", ["2site", "1site"])
def test_holstein_multistate(method):
    """mps/tests/test_gs.py:40-61: state-averaged DMRG, four lowest one-exciton states of the test model."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    model = _holstein_test_model()
    mpo = Mpo(model)
    procedure = [[10, 0.4], [20, 0.2], [30, 0.1], [40, 0], [40, 0]]
    mps = Mps.random(model, 1, procedure[0][0], rng=np.random.default_rng(2019))
    mps.optimize_config.procedure = procedure
    mps.optimize_config.nroots = 4
    mps.optimize_config.method = method
    mps.optimize_config.e_atol = 1e-6
    mps.optimize_config.e_rtol = 1e-6
    energy, states = optimize_mps(mps, mpo)
    energy_std = np.array([0.08401412, 0.08449771, 0.08449801, 0.08449945]) + model.gs_zpe
    assert len(states) == 4
    assert np.allclose(energy[-1], energy_std)
    assert np.allclose([m.expectation(mpo) for m in states], energy_std)
    # the states are orthonormal
    for i, a in enumerate(states):
        for j, b in enumerate(states):
            ov = a.conj().dot(b) if hasattr(a, "conj") else None
            if ov is not None:
                assert abs(ov - (i == j)) < 1e-5


@pytest.mark.parametrize("nroots", [1, 4])
def test_holstein_excited_states_omega(nroots):
    """mps/tests/test_gs.py:64-86 (test_ex): minimising (H - omega)^2 around omega = 0.084 finds the same states."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    model = _holstein_test_model()
    mpo = Mpo(model)
    procedure = [[10, 0.4], [20, 0.2], [30, 0.1], [40, 0], [40, 0]]
    mps = Mps.random(model, 1, procedure[0][0], rng=np.random.default_rng(2019))
    mps.optimize_config.procedure = procedure
    mps.optimize_config.nroots = nroots
    mps.optimize_config.method = "2site"
    mps.optimize_config.e_atol = 1e-6
    mps.optimize_config.e_rtol = 1e-6
    energy, states = optimize_mps(mps, mpo, omega=0.084)
    energy_std = np.array([0.08401412, 0.08449771, 0.08449801, 0.08449945]) + model.gs_zpe
    if nroots == 1:
        assert np.allclose(states.expectation(mpo), energy_std[0])
    else:
        assert np.allclose([m.expectation(mpo) for m in states], energy_std)


def test_mpo_algebra_dense():
    """Mpo.add / scale / product against dense matrices (operator algebra used by the omega functional)."""
    model = _holstein_test_model()
    from renormalizer_amd import Op
    a = Mpo(model, Op(r"a^\dagger a", 0, 0.7))
    b = Mpo(model, Op("x", (1, 0), 1.3))
    h = Mpo(model)
    ident = Mpo.identity(model)
    shifted = h.add(ident.scale(-0.05))
    assert shifted.bond_dims[1:-1] == [w + 1 for w in h.bond_dims[1:-1]]
    # compare through expectation values on a random state (dense matrices of this model are 2^3 4^6 = 32768 wide)
    from renormalizer_amd.mps.mps import Mps
    psi = Mps.random(model, 1, 6, rng=np.random.default_rng(5))
    e = psi.expectation(h)
    assert abs(psi.expectation(shifted) - (e - 0.05)) < 1e-12
    ab = a.product(b)
    phi = b.apply(psi)
    assert abs(psi.expectation(ab) - psi.conj().dot(a.apply(phi))) < 1e-12
    h2 = shifted.product(shifted)
    hpsi = shifted.apply(psi)
    assert abs(psi.expectation(h2) - hpsi.conj().dot(hpsi)) < 1e-10


def test_complex_hopping_ring_ground_state():
    """A real random guess with a complex effective Hamiltonian (Peierls phases on a 4-site ring threaded by a flux):
    the Davidson iteration must promote its vectors (the NumPy reference does so silently, gs.py:520-538)."""
    from renormalizer_amd import BasisSimpleElectron, Op
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    n, phi = 4, 0.37
    basis = [BasisSimpleElectron(i) for i in range(n)]
    terms = []
    for i in range(n):
        j = (i + 1) % n
        terms.append(Op(r"a^\dagger a", [i, j], -1.0 * np.exp(1j * phi)))
        terms.append(Op(r"a^\dagger a", [j, i], -1.0 * np.exp(-1j * phi)))
        terms.append(Op(r"a^\dagger a", [i, i], 0.1 * i))
    model = Model(basis, terms)
    mpo = Mpo(model)
    assert mpo.is_complex
    dense = mpo.todense()
    assert np.abs(dense - dense.conj().T).max() < 1e-14
    bits = (np.arange(2 ** n)[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1
    sector = bits.sum(1) == 1
    exact = np.linalg.eigvalsh(dense[np.ix_(sector, sector)])[0]
    for method in ("1site", "2site"):
        mps = Mps.random(model, 1, 4, rng=np.random.default_rng(3))
        assert not mps.is_complex
        mps.optimize_config.procedure = [[4, 0.2], [4, 0], [4, 0], [4, 0]]
        mps.optimize_config.method = method
        energies, opt = optimize_mps(mps.copy(), mpo)
        assert abs(min(energies) - exact) < 1e-10, (method, energies, exact)
        assert abs(opt.expectation(mpo) - exact) < 1e-9


def test_two_site_dmrg_with_on_the_fly_swapping():
    """gs.py:300-301: two-site DMRG with OFS on the Holstein test Hamiltonian written as a general Model; with a
    bond dimension too small for the original site order the swapped order must not do worse, the returned state and
    the (swapped) MPO stay consistent, and every degree of freedom is still present exactly once"""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    from renormalizer_amd.utils import OFS, CompressConfig, CompressCriteria
    hol = _holstein_test_model()
    results = {}
    for ofs in (None, OFS.ofs_d):
        model = Model(hol.basis, hol.ham_terms)
        mpo = Mpo(model)
        procedure = [[6, 0.4], [6, 0.2], [6, 0.1], [6, 0], [6, 0], [6, 0]]
        mps = Mps.random(model, 1, 6, rng=np.random.default_rng(2019))
        mps.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=6, ofs=ofs)
        mps.optimize_config.procedure = procedure
        mps.optimize_config.method = "2site"
        energies, opt = optimize_mps(mps, mpo)
        assert sorted(map(str, (b.dofs[0] for b in opt.model.basis))) == sorted(map(str, (b.dofs[0] for b in hol.basis)))
        assert abs(opt.expectation(mpo) - energies[-1]) < 1e-8 or abs(opt.expectation(Mpo(opt.model)) - min(energies)) < 1e-6
        assert np.abs(mpo.todense() - Mpo(mpo.model).todense()).max() < 1e-12
        results[ofs] = min(energies)
    exact = 0.0953734687866298
    assert results[OFS.ofs_d] >= exact - 1e-9
    assert results[OFS.ofs_d] <= results[None] + 1e-6


def test_stacked_mpo_seams_match_reference(golden_dir):
    """contract_one_site_multi_mpo (mps/lib.py:121-166) and the two-layer hop_expr (mps/hop_expr.py:24-52) through the
    C ABI against reference-captured inputs / outputs (tests/golden/dmrg_seams.npz): real / complex, L / R, with and
    without ancilla, one- and two-site centres."""
    from renormalizer_amd.engine import get_engine
    from renormalizer_amd.mps.hop_expr import hop_expr
    from renormalizer_amd.mps.lib import contract_one_site_multi_mpo
    eng = get_engine()
    z = np.load(os.path.join(golden_dir, "dmrg_seams.npz"))
    for k in range(int(z["menv_n"])):
        g = lambda n: z[f"menv{k}_{n}"]
        out = contract_one_site_multi_mpo(eng.asdevice(g("env")), eng.asdevice(g("ms")),
                                          [eng.asdevice(g("mo1")), eng.asdevice(g("mo2"))], str(g("dom"))).to_host()
        assert out.shape == g("out").shape
        assert np.abs(out - g("out")).max() < 1e-12 * max(1, np.abs(g("out")).max()), k
    for k in range(int(z["hop2_n"])):
        g = lambda n: z[f"hop2_{k}_{n}"]
        ns = int(g("nsite"))
        hop = hop_expr(g("l"), g("r"), [g(f"w{j}") for j in range(ns)], g("c").shape, True)
        out = hop(eng.asdevice(g("c"))).to_host()
        assert np.abs(out - g("out")).max() < 1e-12 * max(1, np.abs(g("out")).max()), k
        # the dense form used by the direct solver reproduces the action
        dense = hop.dense()
        assert np.abs(dense @ g("c").ravel() - g("out").ravel()).max() < 1e-11 * max(1, np.abs(g("out")).max())


def test_eigensolver_seams_match_reference(golden_dir):
    """eigh_iterative (Davidson in the engine, gs.py:486-576) and eigh_direct (gs.py:383-407) on centre problems
    captured inside the reference's sweeps - (L, W, R, qn_mask, guess) -> (e, c) - for one-layer and (H - omega)^2
    problems, one- and two-site centres.  Eigenvectors agree up to the sign the reference fixes (gs.py:372-380)."""
    import types
    from renormalizer_amd.engine import get_engine
    from renormalizer_amd.mps import gs
    from renormalizer_amd.utils import OptimizeConfig
    eng = get_engine()
    z = np.load(os.path.join(golden_dir, "dmrg_seams.npz"))
    seen = set()
    for k in range(int(z["eig_n"])):
        g = lambda n: z[f"eig{k}_{n}"]
        kind, two, ns = str(g("kind")), bool(g("twolayer")), int(g("nsite"))
        seen.add((kind, two, ns))
        mask = g("mask")
        cmo = [eng.asdevice(g(f"w{j}")) for j in range(ns)]
        mps = types.SimpleNamespace(optimize_config=OptimizeConfig())
        l, r = eng.asdevice(g("l")), eng.asdevice(g("r"))
        if kind == "it":
            guess = np.zeros(mask.shape)
            guess[mask] = g("guess")
            e, c, ncyc = gs.eigh_iterative(mps, mask, l, r, cmo, eng.asdevice(guess), two)
            assert 0 < ncyc < 100
        else:
            e, c, _ = gs.eigh_direct(mps, mask, l, r, cmo, two)
        # Davidson stops at |r| < 1e-6 in both codes: eigenvalues agree to ~|r|^2 / gap
        tol = 2e-9 if kind == "it" else 1e-11
        assert abs(e - float(g("e"))) < tol * max(1.0, abs(float(g("e")))), (k, kind, two, e, float(g("e")))
        cvec = c.to_host()[mask]
        assert np.abs(c.to_host()[~mask]).max() == 0.0
        ref = g("c")
        # eigenvectors of an iteration stopped at |r| < 1e-6 agree to (|r| / gap)^2 in the overlap; the spectrum of
        # (H - omega)^2 is the square of a narrow window around omega, its gaps are correspondingly small
        otol = 1e-10 if kind == "di" else (1e-3 if two else 1e-5)
        assert abs(abs(np.vdot(ref, cvec)) / np.linalg.norm(cvec) - 1.0) < otol, (k, kind, two)
        if kind == "di":
            assert np.abs(cvec - ref).max() < 1e-7                        # same sign convention
    assert {("it", False, 2), ("it", False, 1), ("di", False, 2), ("di", False, 1), ("it", True, 2), ("it", True, 1),
            ("di", True, 1)} <= seen
    # the converged sweep energies of those runs (random starts differ, the fixed points do not)
    for method in ("2site", "1site"):
        assert abs(z[f"holstein_{method}_gs_energies"][-1] - 0.0953734687866) < 2e-9


@pytest.mark.parametrize("method", ["2site", "1site"])
def test_holstein_omega_two_layer_matches_reference(golden_dir, method):
    """optimize_mps(omega=0.09) (gs.py:106-112: two-layer environments) converges to the reference's value of the
    (H - omega)^2 functional for the Holstein test model."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    z = np.load(os.path.join(golden_dir, "dmrg_seams.npz"))
    model = _holstein_test_model()
    mpo = Mpo(model)
    mps = Mps.random(model, 1, 12, rng=np.random.default_rng(2019))
    mps.optimize_config.procedure = [[12, 0.4], [16, 0.2], [20, 0], [20, 0]]
    mps.optimize_config.method = method
    energies, opt = optimize_mps(mps.copy(), mpo, omega=float(z["eig_omega"]))
    ref = float(z[f"holstein_{method}_omega_energies"][-1])
    assert abs(min(energies) - ref) < 1e-9, (energies, ref)
    e = opt.expectation(mpo)
    assert abs((e - 0.09) ** 2 - ref) < 1e-7


def test_h2o_sweep_energies_and_saturated_bonds_match_reference(golden_dir):
    """BASELINE config 5 at its stated size: example/h2o_qc.py from the reference's own seeded random start
    (tests/golden/h2o_dmrg.npz), procedure [[M, .4], [M, .2], [M, .1], [M, 0] x 4] at M = 50 and at M = 512 - the
    exact bond dimensions of 14 spin orbitals with (5, 5) electrons saturate at 37, so both run the same workload
    (SURVEY.md section 8d item 5).  Sweeps with percent = 0 reproduce the reference's energies to 1e-9 and the final
    bond dimensions exactly.  The sweeps with percent > 0 fill their per-block quotas with null-space vectors, which
    the reference draws from numpy's global generator (mps/svd_qn.py:52-63): re-seeding it moves the reference's own
    first-sweep energy by 4e-3 and its second by 1e-8 (``energies_M50_reseeded``), so those two are compared on that
    scale (the null-space completion here is a deterministic Householder basis)."""
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    z = np.load(os.path.join(golden_dir, "h2o_dmrg.npz"))
    sh, aseri, nuc = h_qc.read_fcidump(os.path.join(golden_dir, "h2o_fcidump.txt"), 7)
    model = Model(*h_qc.qc_model(sh, aseri))
    mpo = Mpo(model)
    assert mpo.bond_dims == z["mpo_bond_dims"].tolist()
    n = int(z["init_nsite"])
    for M in (50, 512):
        mps = Mps.from_arrays(model, [z[f"init_site_{i}"] for i in range(n)], [z[f"init_qn_{i}"] for i in range(n + 1)],
                              int(z["init_qnidx"]), z["init_qntot"], bool(z["init_to_right"]), complex(z["init_coeff"]).real)
        mps.optimize_config.procedure = [[M, 0.4], [M, 0.2], [M, 0.1], [M, 0], [M, 0], [M, 0], [M, 0]]
        mps.optimize_config.method = "2site"
        energies, gs_mps = optimize_mps(mps, mpo)
        ref = z[f"energies_M{M}"]
        assert len(energies) == len(ref), (energies, ref)               # same convergence decision (4 sweeps)
        dev = np.abs(np.array(energies) - ref)
        assert dev[0] < 0.05 and dev[1] < 1e-5 and dev[2:].max() < 1e-9, (M, energies, ref)
        spread = np.ptp(z["energies_M50_reseeded"], axis=0)
        assert spread[0] > 1e-3 and spread[2:].max() < 1e-9                 # the reference's own reproducibility
        assert abs(min(energies) + nuc - (-75.008697516450)) < 1e-8
        assert list(gs_mps.bond_dims) == z[f"bond_dims_M{M}"].tolist()
        assert list(mps.bond_dims) == z[f"sweep_bond_dims_M{M}"].tolist()
        assert max(gs_mps.bond_dims) == 37


@pytest.mark.parametrize("nroots,algo", [(10, "davidson"), (12, "primme")])
def test_holstein_multistate_many_roots_vs_dense(nroots, algo, monkeypatch):
    """State-averaged DMRG with 10 roots (default space 12 + 3 * 9 = 39 vectors, 50 with the roots and the new
    direction) and 12 roots with algo = "primme" (space 31, 44 in all): the block Davidson holds that many basis
    vectors, and the converged energies are the lowest eigenvalues of the dense Hamiltonian in the one-exciton sector.
    Three molecules x one mode x six levels: 1728 states, 648 in the sector; the two-site centres of the middle of the
    chain have 1728 elements, so Davidson (not the dense centre solver) does the work there."""
    from renormalizer_amd.mps import gs
    from renormalizer_amd.mps.gs import optimize_mps
    from renormalizer_amd.mps.mps import Mps
    ph = [Phonon.simple_phonon(Quantity(1555.55, "cm^{-1}"), Quantity(8.7729), 6)]
    j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
    model = HolsteinModel([Mol(Quantity(2.67, "eV"), ph, 15.45)] * 3, j, 3)
    mpo = Mpo(model)
    calls = []
    inner = gs.eigh_iterative

    def counted(mps, qn_mask, *args, **kwargs):
        calls.append(int(np.prod(qn_mask.shape)))
        return inner(mps, qn_mask, *args, **kwargs)

    monkeypatch.setattr(gs, "eigh_iterative", counted)
    M = 30
    mps = Mps.random(model, 1, M, rng=np.random.default_rng(2024))
    mps.optimize_config.procedure = [[M, 0.4], [M, 0.2], [M, 0.1], [M, 0], [M, 0], [M, 0]]
    mps.optimize_config.method = "2site"
    mps.optimize_config.nroots = nroots
    mps.optimize_config.algo = algo
    mps.optimize_config.e_atol = 1e-8
    mps.optimize_config.e_rtol = 1e-8
    energies, states = optimize_mps(mps, mpo)
    assert calls            # (only centres of >= 1000 elements reach eigh_iterative)
    assert len(states) == nroots
    dense = mpo.todense()
    nex = np.zeros(dense.shape[0])
    dims = [int(d) for d in model.pbond_list]
    idx = np.indices(dims).reshape(len(dims), -1)
    for site, b in enumerate(model.basis):
        sq = np.asarray(b.sigmaqn).reshape(dims[site], -1)[:, 0]
        nex += sq[idx[site]]
    sector = nex == 1
    assert sector.sum() == 648
    w = np.linalg.eigvalsh(dense[np.ix_(sector, sector)])
    assert np.abs(np.asarray(energies[-1]) - w[:nroots]).max() < 1e-7
