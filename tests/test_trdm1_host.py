"""Host side of the one-site transition density matrices (no GPU): the three exports, the path rule of
``mpse_mps_trdm1_plan`` on dims tables, the checks ``Engine.mps_trdm1`` makes before it calls the library, and the host
arithmetic of ``transport.SpectralFunctionZT``.

LDS plan of either launch (include/mpsengine.h, mpse_mps_trdm1_plan), dims rows (Db_l, Dk_l, d, danc, Db_r, Dk_r), in
working elements of 8 (real) or 16 (complex) bytes: region E, the largest of Db * (Dk | 1) over the bonds and Db_l * Db_r
over the sites, plus region T, the largest of Db_l * (Dk_r | 1) and Dk_l * (Db_r | 1) over the sites.  The launches fit
when the two regions lie within 160 KiB, Db * Dk <= 4096 (1024 threads, 4 accumulators each) at every bond and d, danc, d
* danc <= 65536."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.engine import TRDM1_PLAN_INFO, Engine, check_selection, mps_trdm1_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpse_mps_trdm1", "mpse_mps_trdm1_stats", "mpse_mps_trdm1_plan")


def _table(bra, ket, d=2, danc=1):
    return [[bra[i], ket[i], d, danc, bra[i + 1], ket[i + 1]] for i in range(len(bra) - 1)]


def test_the_three_symbols_everywhere():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mpsengine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mpse_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(E.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in E.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert Engine.TRDM1_STATS == ("chain_kernel", "enqueued", "sites", "matrices")


def test_plan_reports_its_limits():
    ok, info = mps_trdm1_plan(_table((1, 4, 4, 1), (1, 4, 4, 1)), 2, True)
    assert tuple(info) == TRDM1_PLAN_INFO and info["valid"] == 1
    assert info["lds_budget"] == 160 * 1024 and info["threads"] == 1024 and info["acc_limit"] == 4096
    assert info["nsel_limit"] == 0 and info["p_limit"] == 65536
    assert 1 <= info["bond_limit"] <= info["bond_limit_bra1"]
    # by hand: E = max(4 * 5, 4 * 4) = 20, T = max(4 * 5, 4 * 5) = 20; complex (20 + 20) * 16 = 640 bytes, real 320
    assert info["e_elems"] == 20 and info["t_elems"] == 20 and info["lds_fit_bytes"] == 640
    assert ok == (info["bond_limit"] >= 4) and info["lds_bytes"] == (640 if ok else 0)
    assert info["max_bond_bra"] == 4 and info["max_bond_ket"] == 4
    ok_r, real = mps_trdm1_plan(_table((1, 4, 4, 1), (1, 4, 4, 1)), 2, False)
    assert real["lds_fit_bytes"] == 320 and real["lds_bytes"] == (320 if ok_r else 0) and ok_r == ok
    # bra (1, 2, 5, 1) against ket (1, 3, 7, 1).  E: bonds 1 * 1, 2 * 3, 5 * 7 = 35; U of the sites 1 * 2, 2 * 5, 5 * 1.
    # T: site 0: 1 * 3, 1 * 3; site 1: 2 * 7 = 14, 3 * 5 = 15; site 2: 5 * 1, 7 * 1.  (35 + 15) * 16 = 800
    info = mps_trdm1_plan(_table((1, 2, 5, 1), (1, 3, 7, 1)), 1, True)[1]
    assert (info["e_elems"], info["t_elems"], info["lds_fit_bytes"]) == (35, 15, 800)
    assert (info["max_bond_bra"], info["max_bond_ket"]) == (5, 7)
    # swapped: E: 3 * 3 = 9 (pitch of 2 is 3), 7 * 5 = 35; U: 1 * 3, 3 * 7 = 21, 7 * 1.  T: site 0: 1 * 3, 1 * 3; site 1:
    # 3 * 5 = 15, 2 * 7 = 14; site 2: 7 * 1, 5 * 1
    info = mps_trdm1_plan(_table((1, 3, 7, 1), (1, 2, 5, 1)), 1, False)[1]
    assert (info["e_elems"], info["t_elems"], info["lds_fit_bytes"]) == (35, 15, 400)
    assert (info["max_bond_bra"], info["max_bond_ket"]) == (7, 5)


@pytest.mark.parametrize("cplx", (False, True))
def test_rectangular_environments_fit_without_a_bond_cap(cplx):
    es = 16 if cplx else 8
    # Db = 64, Dk = 1: an environment has 64 elements, U of the middle site 64 * 64 = 4096: E = 4096; T = 1 * (64 | 1)
    ok, info = mps_trdm1_plan(_table((1, 64, 64, 1), (1, 1, 1, 1)), 3, cplx)
    assert (info["e_elems"], info["t_elems"], info["lds_fit_bytes"]) == (4096, 65, 4161 * es)
    assert ok == (info["bond_limit"] >= 64) and info["lds_bytes"] == (4161 * es if ok else 0)
    # Db = 1, Dk = 256: E = 1 * 257, U = 1; T = max(1 * 257, 256 * 1)
    ok, info = mps_trdm1_plan(_table((1, 1, 1, 1), (1, 256, 256, 1)), 3, cplx)
    assert (info["e_elems"], info["t_elems"], info["lds_fit_bytes"]) == (257, 257, 514 * es)
    assert ok == (info["bond_limit_bra1"] >= 256) and (info["max_bond_bra"], info["max_bond_ket"]) == (1, 256)
    # both at 64: E = 64 * 65, T = 64 * 65
    info = mps_trdm1_plan(_table((1, 64, 64, 1), (1, 64, 64, 1)), 3, cplx)[1]
    assert (info["e_elems"], info["t_elems"], info["lds_fit_bytes"]) == (4160, 4160, 8320 * es)
    # at the rule's limit on both chains the kernels take the call, one above on either chain they do not
    lim = info["bond_limit"]
    assert mps_trdm1_plan(_table((1, lim, lim, 1), (1, lim, lim, 1)), 3, cplx)[0]
    for bra, ket in (((1, lim + 1, lim, 1), (1, lim, lim, 1)), ((1, 2, 2, 1), (1, lim, lim + 1, 1))):
        ok, info = mps_trdm1_plan(_table(bra, ket), 3, cplx)
        assert not ok and info["valid"] == 1 and info["lds_bytes"] == 0 and info["lds_fit_bytes"] > 0
    lim1 = info["bond_limit_bra1"]
    assert mps_trdm1_plan(_table((1, 1, 1, 1), (1, lim1, lim1, 1)), 3, cplx)[0]
    assert not mps_trdm1_plan(_table((1, 1, 1, 1), (1, lim1, lim1 + 1, 1)), 3, cplx)[0]


def test_one_accumulator_per_entry_and_the_lds_budget():
    # 16 * 256 = 4096 entries: fits.  E = max(16 * 257, 16 * 16) = 4112, T = max(16 * 257, 256 * 17) = 4352
    info = mps_trdm1_plan(_table((1, 16, 16, 1), (1, 256, 256, 1)), 3, True)[1]
    assert (info["e_elems"], info["t_elems"], info["lds_fit_bytes"]) == (4112, 4352, 8464 * 16)
    # 17 * 241 = 4097 entries, one above the accumulators; its regions (4114 + 4338 elements) would lie inside the LDS
    for bra, ket in (((1, 17, 17, 1), (1, 241, 241, 1)), ((1, 241, 241, 1), (1, 17, 17, 1)), ((1, 17, 1), (1, 241, 1))):
        ok, info = mps_trdm1_plan(_table(bra, ket), 1, True)
        assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["e_elems"] == 0
    # Db = 2, Dk = 2048 has its 4096 entries, E = 2 * 2049 = 4098, T = max(2 * 2049, 2048 * 3) = 6144: 10242 elements are
    # 81 936 bytes real and 163 872 complex, 32 above the 163 840 of the budget
    ok, info = mps_trdm1_plan(_table((1, 2, 2, 1), (1, 2048, 2048, 1)), 3, False)
    assert (info["e_elems"], info["t_elems"], info["lds_fit_bytes"]) == (4098, 6144, 81936)
    ok, info = mps_trdm1_plan(_table((1, 2, 2, 1), (1, 2048, 2048, 1)), 3, True)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["max_bond_ket"] == 2048


def test_physical_extent_over_the_limit():
    one = (1, 1, 1)
    assert mps_trdm1_plan(_table(one, one, d=65536), 1, False)[0]
    assert mps_trdm1_plan(_table(one, one, d=256, danc=256), 1, False)[0]
    for d, danc in ((65537, 1), (256, 257), (1, 65537)):
        ok, info = mps_trdm1_plan(_table(one, one, d=d, danc=danc), 1, False)
        assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0


def test_tables_that_are_no_chain():
    good = _table((1, 1, 1, 1), (1, 1, 1, 1))
    assert mps_trdm1_plan(good, 2, True)[0]
    # first bond, last bond, a neighbour and an empty extent, in the bra's columns (0, 4) and in the ket's (1, 5)
    for i, j, v in ((0, 0, 2), (0, 1, 2), (2, 4, 2), (2, 5, 2), (1, 0, 4), (1, 1, 4), (1, 4, 3), (1, 5, 3), (1, 2, 0),
                    (1, 3, 0), (2, 5, -1)):
        bad = [list(r) for r in good]
        bad[i][j] = v
        ok, info = mps_trdm1_plan(bad, 2, True)
        assert not ok and info["valid"] == 0 and info["max_bond_bra"] == 0 and info["max_bond_ket"] == 0, bad
    assert not mps_trdm1_plan([], 1, True)[0] and mps_trdm1_plan([], 1, True)[1]["valid"] == 0


def test_empty_selection():
    tab = _table((1, 2, 1), (1, 2, 1))
    assert mps_trdm1_plan(tab, 1, True)[0] and mps_trdm1_plan(tab, 300, True)[0]      # no cap on the selection
    ok, info = mps_trdm1_plan(tab, 0, True)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0
    assert not mps_trdm1_plan(tab, -1, True)[0]


def test_square_tables_are_sized_as_one_chain():
    """ONE chain is the case bra = ket of two: on seeded random square tables ``mps_rdm1_plan`` of the rows (D_l, d,
    danc, D_r) and ``mps_trdm1_plan`` of the same rows written with six columns agree on the path, the LDS bytes and
    elements, the largest bond and ``valid``.  1 .. 7 sites, bonds up to 128, d up to 70000, real and complex, so that
    tables the kernels take, tables that only fit and tables that do not fit all occur."""
    from renormalizer_amd.engine import mps_rdm1_plan
    rng = np.random.default_rng(20240611)
    taken = fit_only = no_fit = 0
    for _ in range(400):
        nsite = int(rng.integers(1, 8))
        cap = int(rng.choice((1, 4, 16, 64, 128)))
        bonds = [1] + [int(rng.integers(1, cap + 1)) for _ in range(nsite - 1)] + [1]
        dims4 = []
        for i in range(nsite):
            d = int(rng.choice((65536, 70000))) if rng.random() < 0.05 else int(rng.integers(1, 9))
            dims4.append([bonds[i], d, int(rng.integers(1, 3)), bonds[i + 1]])
        if rng.random() < 0.05:
            dims4[0][0] = 2                                              # no chain: both report valid = 0
        dims6 = [[r[0], r[0], r[1], r[2], r[3], r[3]] for r in dims4]
        nsel, cplx = int(rng.integers(0, nsite + 1)), bool(rng.integers(0, 2))
        ok1, one = mps_rdm1_plan(dims4, nsel, cplx)
        ok2, two = mps_trdm1_plan(dims6, nsel, cplx)
        assert ok1 == ok2, (dims4, nsel, cplx)
        for name in ("lds_bytes", "lds_fit_bytes", "e_elems", "t_elems", "valid"):
            assert one[name] == two[name], (name, dims4, nsel, cplx)
        assert one["max_bond"] == two["max_bond_bra"] == two["max_bond_ket"], (dims4, nsel, cplx)
        taken += ok1
        fit_only += (not ok1) and one["lds_fit_bytes"] > 0
        no_fit += one["valid"] == 1 and one["lds_fit_bytes"] == 0
    assert taken > 0 and fit_only > 0 and no_fit > 0, (taken, fit_only, no_fit)


def test_binding_refuses_before_the_library():
    def z(*shape):
        return np.zeros(shape)

    good = [z(1, 2, 3), z(3, 2, 1)]
    assert Engine.trdm1_dims(good, [z(1, 2, 5), z(5, 2, 1)]) == [[1, 1, 2, 1, 3, 5], [3, 5, 2, 1, 1, 1]]
    assert Engine.trdm1_dims([z(1, 2, 4, 3)], [z(2, 2, 4, 1)]) == [[1, 2, 2, 4, 3, 1]]
    for bra, ket in ((good, good[:1]),                                   # chains of different length
                     ([], []),                                           # an empty chain
                     ([z(1, 2), z(2, 2, 1)], good),                      # a site of rank 2
                     (good, [z(1, 2, 1, 1, 3), z(3, 2, 1)]),             # a site of rank 5
                     (good, [z(1, 3, 3), z(3, 2, 1)]),                   # physical extents differ
                     ([z(1, 2, 2, 3), z(3, 2, 2, 1)], [z(1, 2, 3, 3), z(3, 2, 3, 1)]),   # ancilla extents differ
                     ([z(1, 2, 2, 3), z(3, 2, 1)], good)):               # an ancilla leg on one side only
        with pytest.raises(ValueError):
            Engine.trdm1_dims(bra, ket)
    for sel, n in (((2, 0), 3), ((1, 1), 3), ((0, 3), 3), ((-1, 1), 3), ((), 3)):
        with pytest.raises(ValueError):
            check_selection("mps_trdm1", sel, n)


def _model(ncell=4):
    from renormalizer_amd.model.basis import BasisSHO, BasisSimpleElectron
    from renormalizer_amd.model.model import TI1DModel
    from renormalizer_amd.model.op import Op
    basis = [BasisSimpleElectron("e"), BasisSHO("ph", 1.0, 2)]
    local = [Op(r"b^\dagger b", "ph", 1.0)]
    hopping = [Op(r"a^\dagger a", [(0, "e"), (1, "e")], 0.5), Op(r"a^\dagger a", [(1, "e"), (0, "e")], 0.5)]
    return TI1DModel(basis, local, hopping, ncell)


def test_job_is_exported_and_dumps_the_reference_keys():
    from renormalizer_amd import transport
    from renormalizer_amd.utils import Quantity
    assert "SpectralFunctionZT" in transport.__all__
    job = transport.SpectralFunctionZT.__new__(transport.SpectralFunctionZT)     # no state, no GPU: the host arithmetic
    job.model = _model(4)
    job.temperature = Quantity(0)
    job.evolve_times = [0, 0.5, 1.0]
    rng = np.random.default_rng(5)
    g = rng.standard_normal((3, 4)) + 1j * rng.standard_normal((3, 4))
    job._G_array = [row for row in g]
    job.e_occupations_array = [np.full(4, 0.25)] * 3
    dump = job.get_dump_dict()
    assert list(dump) == ["temperature", "time series", "G array", "Gk array", "electron occupations array"]
    assert dump["temperature"] == 0 and dump["time series"] == [0, 0.5, 1.0]
    assert np.array_equal(dump["G array"], g) and np.array_equal(job.G_array, g)
    # G_k(t) = sum_d G_d(t) exp(i k d) for k = 0, pi / 2, pi: ne // 2 + 1 = 3 points of spacing 2 pi / 4
    gk = np.array([[sum(g[t, dd] * np.exp(1j * (2 * np.pi / 4) * k * dd) for dd in range(4)) for k in range(3)]
                   for t in range(3)])
    assert dump["Gk array"].shape == (3, 3) and np.abs(dump["Gk array"] - gk).max() < 1e-14
    assert np.abs(dump["Gk array"][:, 0] - g.sum(axis=1)).max() < 1e-14
