"""Host side of ``mpse_mps_expect_many``, ``Property``, ``property.ops`` and ``ThermalProp`` (no GPU): the path rule of
``mpse_mps_expect_many_plan`` on dims tables, the bookkeeping of ``Property`` against a stub state that records its
calls, the operators of ``ops`` against ``numpy.kron``, and the keys of the job's dump."""
import numpy as np
import pytest

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity
from renormalizer_amd.engine import mps_expect_many_plan
from renormalizer_amd.model.op import Op
from renormalizer_amd.mps import ThermalProp
from renormalizer_amd.property import Property, ops


def _table(bonds, d=2, danc=1):
    return [[bonds[i], d, danc, bonds[i + 1]] for i in range(len(bonds) - 1)]


def _window(first, bonds):
    """(first site, [(wl, wr)]) of a window whose MPO bonds are ``bonds`` (1 at both ends)"""
    return first, [(bonds[i], bonds[i + 1]) for i in range(len(bonds) - 1)]


# ---------------------------------------------------------------------------------------------- path rule
def test_plan_sizes_by_hand():
    tab = _table((1, 4, 4, 1))
    wins = [_window(0, (1, 3, 1)), _window(2, (1, 1))]
    ok, info = mps_expect_many_plan(tab, wins, True)
    assert ok and info["valid"] == 1
    assert info["lds_budget"] == 160 * 1024 and info["threads"] == 1024 and info["bond_fit_limit"] == 64
    assert 1 <= info["bond_limit"] <= info["bond_fit_limit"]              # the rule's limit is a measured one
    assert info["grid_cap"] >= 64 and info["channel_limit"] == 8 and info["acc_per_thread"] == 16
    # the walks: L or R of bond 4 as 4 rows of pitch 5, T of site 1 the same
    assert info["e_elems"] == 20 and info["t_elems"] == 20
    # the windows: E (4, 3, 4) behind site 0 is 12 rows of pitch 5; T of site 1 is D_l wl D_r = 4 * 3 * 4
    assert info["win_e_elems"] == 60 and info["win_t_elems"] == 48 and info["w_max"] == 3
    assert info["acc_needed"] == 8                                         # 16 entries of a plane: one per thread, 8 channels
    # the larger launch is the second one: E, T and 16 reduction words, complex
    assert info["lds_bytes"] == (60 + 48 + 16) * 16 == info["lds_fit_bytes"] and info["elem_bytes"] == 16
    assert info["max_bond"] == 4
    info = mps_expect_many_plan(tab, wins, False)[1]
    assert info["lds_bytes"] == (60 + 48 + 16) * 8 and info["elem_bytes"] == 8
    # with bond-1 MPOs the window launch is E (20) + T (16) + 16 words, the walks need 40
    assert mps_expect_many_plan(tab, [_window(1, (1, 1))], True)[1]["lds_bytes"] == (20 + 16 + 16) * 16


@pytest.mark.parametrize("cplx", (False, True))
def test_state_bond_at_the_limit_and_above(cplx):
    limit = mps_expect_many_plan(_table((1, 1)), [_window(0, (1, 1))], cplx)[1]["bond_limit"]
    wins = [_window(0, (1, 1, 1, 1)), _window(1, (1, 1))]
    ok, info = mps_expect_many_plan(_table((1, limit, limit, 1)), wins, cplx)
    assert ok and info["max_bond"] == limit and 0 < info["lds_bytes"] <= info["lds_budget"]
    ok, info = mps_expect_many_plan(_table((1, limit, limit + 1, 1)), wins, cplx)
    assert not ok and info["valid"] == 1 and info["lds_bytes"] == 0 and info["max_bond"] == limit + 1
    # above the rule's limit the launches may still fit (MPSE_EXPECT_CHAIN=1 runs them): as long as a bond plane is
    # within the two entries per thread of the site step, 45 * 45 <= 2048 < 46 * 46
    if limit + 1 <= 45:
        assert info["lds_fit_bytes"] > 0
    ok, info = mps_expect_many_plan(_table((1, 45, 46, 1)), wins, cplx)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["acc_needed"] == 24


def test_mpo_bond_at_the_channel_limit_and_above():
    tab = _table((1, 3, 3, 1))
    ok, info = mps_expect_many_plan(tab, [_window(0, (1, 8, 8, 1))], True)
    assert ok and info["w_max"] == 8 == info["channel_limit"]
    ok, info = mps_expect_many_plan(tab, [_window(0, (1, 8, 9, 1))], True)
    assert not ok and info["valid"] == 1 and info["w_max"] == 9 and info["lds_fit_bytes"] == 0
    # one operator over the limit sends the whole call to the enqueued path
    ok, info = mps_expect_many_plan(tab, [_window(1, (1, 1)), _window(1, (1, 9, 1))], True)
    assert not ok and info["valid"] == 1


def test_tables_and_windows_that_are_refused():
    good, win = _table((1, 3, 2, 1)), [_window(0, (1, 2, 1))]
    assert mps_expect_many_plan(good, win, True)[0]
    for i, j, v in ((0, 0, 2), (2, 3, 2), (1, 0, 4), (1, 1, 0), (2, 3, -1)):
        bad = [list(r) for r in good]
        bad[i][j] = v
        ok, info = mps_expect_many_plan(bad, win, True)
        assert not ok and info["valid"] == 0 and info["max_bond"] == 0, bad
    assert mps_expect_many_plan([], win, True)[1]["valid"] == 0
    for wins in ([(1, [])],                          # first > last: a window without sites
                 [_window(3, (1, 1))],               # outside the chain
                 [_window(2, (1, 2, 1))],            # runs over the end
                 [_window(-1, (1, 1))],
                 [(0, [(1, 2), (3, 1)])],            # MPO bonds that do not match
                 [(0, [(2, 1)])], [(0, [(1, 2)])],   # do not start / end at 1
                 []):                                # no operator
        ok, info = mps_expect_many_plan(good, wins, True)
        assert not ok and info["valid"] == 0, wins


# ---------------------------------------------------------------------------------------------- Property
@pytest.fixture(scope="module")
def model3():
    ph = Phonon.simple_phonon(Quantity(0.01), Quantity(2.0), 3)
    return HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(0.02), 3)


class _State:
    """records its calls; the value of an operator is its position in ``book``"""

    def __init__(self, book, offset=0.0):
        self.book, self.offset, self.calls = book, offset, []

    def _value(self, mpo):
        return self.offset + [k for k, m in enumerate(self.book) if m is mpo][0]

    def mpo_expectations(self, mpos):
        self.calls.append(("mpo_expectations", list(mpos)))
        return np.array([self._value(m) for m in mpos])

    def expectation(self, mpo, conj=None):
        self.calls.append(("expectation", mpo, conj))
        return 100.0 + self._value(mpo)

    def edof_rdm(self):
        self.calls.append(("edof_rdm",))
        return np.eye(3)

    def matrix_element(self, mpo, ket, self_is_conj=True):
        self.calls.append(("matrix_element", mpo, ket, self_is_conj))
        return 0.5 - 2.0j


def test_property_gathers_one_call_per_step(model3):
    book = [Mpo(model3, Op(r"a^\dagger a", i)) for i in range(3)] + [Mpo(model3, Op("n", (i, 0))) for i in range(3)]
    prop = Property(["single", "e_rdm", "list", "other"],
                    {"single": book[4], "list": [book[2], book[0], book[5]], "other": book[1]})
    assert prop.prop_res == {"single": [], "e_rdm": [], "list": [], "other": []}
    state = _State(book)
    for step in range(2):
        prop.calc_properties(state)
        gathered = [c for c in state.calls if c[0] == "mpo_expectations"]
        assert len(gathered) == step + 1 and len(state.calls) == 2 * (step + 1)     # and one edof_rdm
        assert [m is n for m, n in zip(gathered[-1][1], [book[4], book[2], book[0], book[5], book[1]])] == [True] * 5
    assert prop.prop_res["single"] == [4.0, 4.0] and prop.prop_res["other"] == [1.0, 1.0]
    assert all(isinstance(v, np.ndarray) and v.tolist() == [2.0, 0.0, 5.0] for v in prop.prop_res["list"])
    assert all(np.array_equal(v, np.eye(3)) for v in prop.prop_res["e_rdm"])
    # a separate bra: one expectation per operator, lists are not taken
    bra = object()
    single = Property(["single", "other"], {"single": book[4], "other": book[1]})
    state = _State(book)
    single.calc_properties(state, bra)
    assert state.calls == [("expectation", book[4], bra), ("expectation", book[1], bra)]
    assert single.prop_res == {"single": [104.0], "other": [101.0]}
    with pytest.raises(AssertionError):
        prop.calc_properties(_State(book), bra)
    with pytest.raises(NotImplementedError):
        Property(["unknown"], {}).calc_properties(_State(book))


def test_property_braketpair_branches(model3):
    book = [Mpo(model3, Op(r"a^\dagger a", i)) for i in range(3)] + [Mpo(model3, Op("x", (0, 0)))]

    class _Pair:
        pass

    pair = _Pair()
    pair.bra_mps, pair.ket_mps = _State(book, 10.0), _State(book, 20.0)
    prop = Property(["n", "j", "x"], {"n": book[:3], "j": book[1], "x": book[3]})
    prop.calc_properties_braketpair(pair)
    (n_val,), (j_val,), (x_val,) = prop.prop_res["n"], prop.prop_res["j"], prop.prop_res["x"]
    assert len(n_val) == 2 and n_val[0].tolist() == [10.0, 11.0, 12.0] and n_val[1].tolist() == [20.0, 21.0, 22.0]
    assert x_val == [13.0, 23.0]
    assert j_val == 0.5 - 2.0j
    # one gathered call per state; the bra-ket element through the bra, as it is (not conjugated again)
    assert [c[0] for c in pair.bra_mps.calls] == ["mpo_expectations", "matrix_element"]
    assert [c[0] for c in pair.ket_mps.calls] == ["mpo_expectations"]
    assert pair.bra_mps.calls[1][1] is book[1] and pair.bra_mps.calls[1][2] is pair.ket_mps
    assert pair.bra_mps.calls[1][3] is True


# ---------------------------------------------------------------------------------------------- ops
def _dense_product(model, local):
    """kron over the sites of ``local[site]`` (identity elsewhere)"""
    dense = np.ones((1, 1))
    for i, d in enumerate(model.pbond_list):
        dense = np.kron(dense, local.get(i, np.eye(d)))
    return dense


def _n_x(model, imol, jmol):
    ph = model[jmol].ph_list[0]
    n_mat = np.diag([0.0, 1.0])
    d = ph.n_phys_dim
    b = np.diag(np.sqrt(np.arange(1, d)), 1)
    scale = np.sqrt(1.0 / 2.0 / ph.omega[0]) / ph.dis[1]
    return scale * _dense_product(model, {model.dof_to_siteidx[imol]: n_mat, model.dof_to_siteidx[(jmol, 0)]: b + b.T})


def test_static_correlation_operators(model3):
    names = []
    for imol in range(3):
        mpos = ops.e_ph_static_correlation(model3, imol=imol)
        assert list(mpos) == [f"S_{imol}_{j}_0" for j in range(3)]
        names += list(mpos)
        for jmol in range(3):
            assert np.abs(mpos[f"S_{imol}_{jmol}_0"].todense() - _n_x(model3, imol, jmol)).max() <= 1e-15
    assert len(set(names)) == 9
    per = ops.e_ph_static_correlation(model3, periodic=True, name="C")
    assert list(per) == ["C_0_0", "C_1_0", "C_2_0"]
    for dis in range(3):
        total = sum(_n_x(model3, j, (j + dis) % 3) for j in range(3))
        assert np.abs(per[f"C_{dis}_0"].todense() - total).max() <= 1e-15 * 3
    with pytest.raises(NotImplementedError):
        ops.e_ph_static_correlation(model3.switch_scheme(4))


def test_coordinate_operators(model3):
    x, x2 = ops.x_average(model3), ops.x_square_average(model3)
    assert list(x) == ["x"] and list(x2) == ["x^2"]
    assert isinstance(x2["x^2"], list) and len(x["x"]) == len(x2["x^2"]) == len(model3.v_dofs) == 3
    for k, dof in enumerate(model3.v_dofs):
        assert np.array_equal(x["x"][k].todense(), Mpo(model3, Op("x", dof)).todense())
        assert np.array_equal(x2["x^2"][k].todense(), Mpo(model3, Op("x^2", dof)).todense())
    Property(["x^2"], x2)                                     # the value is what Property takes


# ---------------------------------------------------------------------------------------------- the job's dump
REFERENCE_DUMP_KEYS = ["time series", "energies", "electron occupations array", "phonon occupations array",
                       "vn entropy array"]


def test_dump_keys(model3):
    job = ThermalProp.__new__(ThermalProp)                    # no state, no device: the dump alone
    job.evolve_times = [0, -0.5j, -1.0j]
    job.energies = [0.0, -0.1, -0.2]
    job._e_occupations_array = [np.zeros(3)] * 3
    job._ph_occupations_array = [np.zeros(3)] * 3
    job._vn_entropy_array = [np.zeros(5)] * 3
    job.properties = None
    assert list(job.get_dump_dict()) == REFERENCE_DUMP_KEYS
    assert job.get_dump_dict()["time series"] == [0, 0.5, 1.0]
    assert job.e_occupations_array.shape == (3, 3) and job.vn_entropy_array.shape == (3, 5)
    job.properties = Property(["S_0_0", "e_rdm"], {})
    job.properties.prop_res["S_0_0"] = [1.0, 2.0, 3.0]
    dump = job.get_dump_dict()
    assert list(dump) == REFERENCE_DUMP_KEYS + ["S_0_0", "e_rdm"] and dump["S_0_0"] == [1.0, 2.0, 3.0]
    import renormalizer_amd
    assert renormalizer_amd.ThermalProp is ThermalProp and renormalizer_amd.Property is Property
