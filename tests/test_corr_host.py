"""Host side of the correlation matrix and of ``ChargeDiffusionDynamics`` (no GPU): the path rule of
``mpse_mps_corr_plan`` on dims tables, the arithmetic the job does on the electron's density matrix, the local matrices
``Mps.correlation_matrix`` hands to the engine, and the keys of the job's dump."""
import numpy as np
import pytest

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity
from renormalizer_amd.engine import mps_corr_plan
from renormalizer_amd.model.op import Op
from renormalizer_amd.transport import ChargeDiffusionDynamics, EDGE_THRESHOLD, InitElectron, calc_r_square
from renormalizer_amd.transport.dynamics import coherent_length, eph_vn_entropy, k_occupations


def _table(bonds, d=2, danc=1):
    return [[bonds[i], d, danc, bonds[i + 1]] for i in range(len(bonds) - 1)]


# ---------------------------------------------------------------------------------------------- path rule
def test_plan_reports_its_limits():
    ok, info = mps_corr_plan(_table((1, 4, 4, 1)), 2, True)
    assert ok and info["valid"] == 1
    # 160 KiB hold two padded complex 64 x 65 arrays and the reduction words, not two of 128 x 129
    assert info["lds_budget"] == 160 * 1024 and info["bond_fit_limit"] == 64 and info["threads"] == 1024
    assert 1 <= info["bond_limit"] <= info["bond_fit_limit"]              # the rule's limit is a measured one
    assert 2 * 64 * 65 * 16 <= info["lds_budget"] < 2 * 128 * 129 * 16
    assert info["nsel_limit"] >= 64 and info["p_limit"] == 65536
    # E: 4 rows of pitch 5; T: 4 rows of pitch 5; 16 reduction words; complex
    assert info["e_elems"] == 20 and info["t_elems"] == 20 and info["lds_bytes"] == (20 + 20 + 16) * 16
    assert info["lds_fit_bytes"] == info["lds_bytes"]
    assert info["max_bond"] == 4
    assert mps_corr_plan(_table((1, 4, 4, 1)), 2, False)[1]["lds_bytes"] == (20 + 20 + 16) * 8


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(cplx):
    limit = mps_corr_plan(_table((1, 1)), 1, cplx)[1]["bond_limit"]
    ok, info = mps_corr_plan(_table((1, limit, limit, limit, 1)), 3, cplx)
    assert ok and info["max_bond"] == limit
    assert info["e_elems"] == limit * (limit + 1) and info["t_elems"] == limit * (limit + 1)
    assert 0 < info["lds_bytes"] <= info["lds_budget"]
    ok, info = mps_corr_plan(_table((1, limit, limit + 1, limit, 1)), 3, cplx)
    assert not ok and info["valid"] == 1 and info["lds_bytes"] == 0 and info["max_bond"] == limit + 1
    # what the LDS allows is a second, wider limit: launches up to it fit (MPSE_CORR_CHAIN=1 runs them), none above
    fit = info["bond_fit_limit"]
    assert (info["lds_fit_bytes"] > 0) == (limit + 1 <= fit)
    ok, info = mps_corr_plan(_table((1, fit, fit, fit, 1)), 3, cplx)
    assert ok == (fit <= limit) and info["lds_fit_bytes"] == (2 * fit * (fit + 1) + 16) * (16 if cplx else 8)
    assert info["lds_fit_bytes"] <= info["lds_budget"] and info["e_elems"] == fit * (fit + 1)
    ok, info = mps_corr_plan(_table((1, fit, fit + 1, fit, 1)), 3, cplx)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["e_elems"] == 0


def test_physical_extent_over_the_limit():
    assert mps_corr_plan(_table((1, 2, 1), d=65536), 1, False)[0]
    assert mps_corr_plan(_table((1, 2, 1), d=256, danc=256), 1, False)[0]
    for d, danc in ((65537, 1), (256, 257), (1, 65537)):
        ok, info = mps_corr_plan(_table((1, 2, 1), d=d, danc=danc), 1, False)
        assert not ok and info["valid"] == 1


def test_tables_that_are_no_chain():
    good = _table((1, 3, 2, 1))
    assert mps_corr_plan(good, 2, True)[0]
    for i, j, v in ((0, 0, 2), (2, 3, 2), (1, 0, 4), (1, 1, 0), (1, 2, 0), (2, 3, -1)):
        bad = [list(r) for r in good]
        bad[i][j] = v
        ok, info = mps_corr_plan(bad, 2, True)
        assert not ok and info["valid"] == 0 and info["max_bond"] == 0, bad
    assert not mps_corr_plan([], 1, True)[0] and mps_corr_plan([], 1, True)[1]["valid"] == 0


def test_selection_count_at_the_cap_and_over():
    cap = mps_corr_plan(_table((1, 1)), 1, True)[1]["nsel_limit"]
    tab = _table((1,) + (2,) * (cap + 1) + (1,))          # cap + 2 sites
    assert mps_corr_plan(tab, cap, True)[0]
    ok, info = mps_corr_plan(tab, cap + 1, True)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0
    assert not mps_corr_plan(tab, 0, True)[0]


# ---------------------------------------------------------------------------------------------- arithmetic on rho
def test_r_square_by_hand():
    assert calc_r_square([0, 0, 0, 0]) == 0
    assert calc_r_square([0, 1, 0]) == 0.0
    assert calc_r_square([0.5, 0, 0.5]) == pytest.approx(1.0)            # <r^2> = 2, <r> = 1
    assert calc_r_square([0.25, 0.5, 0.25]) == pytest.approx(0.5)
    assert calc_r_square([0.2, 0.4, 0.2]) == pytest.approx(0.5)          # weights need not be normalised
    assert calc_r_square([0, 0, 0.5, 0, 0.5]) == pytest.approx(1.0)      # no dependence on the origin


def test_k_space_occupations():
    rng = np.random.default_rng(3)
    n = 5
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    rho = a @ a.conj().T
    occ = k_occupations(rho)
    ks = -np.pi + 2 * np.pi / n * np.arange(n)
    for k, o in zip(ks, occ):
        vec = np.exp(-1j * k * np.arange(n)) / np.sqrt(n)               # <k|j> of |k> = sum_j exp(-i j k) |j> / sqrt(n)
        assert o == pytest.approx((vec @ rho @ vec.conj()).real, abs=1e-12)
    assert occ.sum() == pytest.approx(np.trace(rho).real)
    # a plane wave sits in one k
    j = np.arange(6)
    psi = np.exp(1j * (2 * np.pi / 6) * j) / np.sqrt(6)
    occ = k_occupations(np.outer(psi.conj(), psi))                       # rho_ij = <a_i^+ a_j> = conj(psi_i) psi_j
    assert np.sort(occ)[-1] == pytest.approx(1.0) and np.sort(occ)[-2] == pytest.approx(0.0, abs=1e-12)


def test_coherence_length_and_entropy():
    assert coherent_length(np.diag([0.2, 0.5, 0.3])) == 0.0
    psi = np.ones(4) / 2
    rho = np.outer(psi.conj(), psi)
    assert coherent_length(rho) == pytest.approx(3.0)                    # 12 off-diagonal entries of 1/4
    assert eph_vn_entropy(rho) == pytest.approx(0.0, abs=1e-12)           # a pure state
    assert eph_vn_entropy(np.eye(4) / 4) == pytest.approx(np.log(4))


# ---------------------------------------------------------------------------------------------- local matrices
@pytest.fixture(scope="module")
def model3():
    ph = Phonon.simple_phonon(Quantity(0.01), Quantity(2.0), 3)
    return HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(0.02), 3)


def _bare_mps(model):
    from renormalizer_amd.mps.mps import Mps
    m = Mps()
    m.model = model
    return m


def test_one_site_operator_is_the_identity_elsewhere(model3):
    for sym, dof in ((r"a^\dagger", 1), ("a", 2), (r"b^\dagger", (0, 0)), ("b", (2, 0)), (r"a^\dagger a", 0)):
        mpo = Mpo(model3, Op(sym, dof))
        site = model3.dof_to_siteidx[dof]
        assert list(mpo.bond_dims) == [1] * (model3.nsite + 1)
        for i in range(model3.nsite):
            w = np.asarray(mpo[i])[0, :, :, 0]
            assert (i == site) or np.array_equal(w, np.eye(w.shape[0])), (sym, dof, i)
        idx, mat = _bare_mps(model3)._local_matrix(sym, dof)
        assert idx == site and np.array_equal(mat, np.asarray(mpo[site])[0, :, :, 0])
    idx, up = _bare_mps(model3)._local_matrix(r"a^\dagger", 0)
    assert np.array_equal(up, np.array([[0.0, 0.0], [1.0, 0.0]]))          # <1| a^+ |0>: the first index is the bra's


def test_local_matrices_build_the_pair_operator(model3):
    mps = _bare_mps(model3)
    dims = model3.pbond_list
    for d1, d2 in ((0, 2), (1, 2), (2, 0), (1, 1)):
        ref = Mpo(model3, Op(r"a^\dagger a", [d1, d2])).todense()
        prod = (Mpo(model3, Op(r"a^\dagger", d1)) @ Mpo(model3, Op("a", d2))).todense()
        assert np.array_equal(prod, ref)
        (s1, m1), (s2, m2) = mps._local_matrix(r"a^\dagger", d1), mps._local_matrix("a", d2)
        dense = np.ones((1, 1))
        for i, d in enumerate(dims):
            local = np.eye(d)
            if i == s1:
                local = local @ m1
            if i == s2:
                local = local @ m2
            dense = np.kron(dense, local)
        assert np.array_equal(dense, ref)


# ---------------------------------------------------------------------------------------------- the job's dump
REFERENCE_DUMP_KEYS = ["mol list", "tempearture", "total time", "other info", "r square array",
                       "electron occupations array", "phonon occupations array", "k occupations array", "eph entropy",
                       "bond entropy", "coherent length array", "reduced density matrices", "time series"]


def test_dump_keys(model3):
    job = ChargeDiffusionDynamics.__new__(ChargeDiffusionDynamics)       # no state, no device: the dump alone
    job.model, job.temperature = model3, Quantity(0, "K")
    job.evolve_times = [0, 2.0]
    for name in ("r_square_array", "e_occupations_array", "ph_occupations_array", "k_occupations_array",
                 "eph_vn_entropy_array", "bond_vn_entropy_array", "coherent_length_array", "energies"):
        setattr(job, name, [0.0, 0.0])
    job.custom_dump_info = {}
    job.reduced_density_matrices = [np.eye(3), np.eye(3)]
    assert list(job.get_dump_dict()) == REFERENCE_DUMP_KEYS
    job.reduced_density_matrices = None                                   # rdm=False: the key is left out
    assert list(job.get_dump_dict()) == [k for k in REFERENCE_DUMP_KEYS if k != "reduced density matrices"]
    assert job.get_dump_dict()["total time"] == 2.0
    assert EDGE_THRESHOLD == 1e-4 and {e.name for e in InitElectron} == {"fc", "relaxed"}
