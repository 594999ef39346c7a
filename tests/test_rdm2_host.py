"""Host side of the two-site density matrices (no GPU): the path rule of ``mpse_mps_rdm2_plan`` on dims tables and
selections, and the checks ``Engine.mps_rdm2`` makes before it calls the library.

LDS plan of either launch (renormalizer_amd/csrc/mpse_rdm2.hip), as for ``mpse_mps_rdm1``: region E, the largest D *
(D | 1) over the bonds, plus region T, the largest D_l * (D_r | 1) over the sites, in working elements of 8 (real) or 16
(complex) bytes.  The second launch has one workgroup per (k, p, p'), k a selected site but the last; the result holds
d_k^2 d_l^2 complex elements per pair."""
import ctypes as C
import os
import re

import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.engine import RDM1_PLAN_INFO, RDM2_PLAN_INFO, check_selection, mps_rdm1_plan, mps_rdm2_plan

NAMES = ("mpse_mps_rdm2", "mpse_mps_rdm2_stats", "mpse_mps_rdm2_plan")


def _table(bonds, d=2, danc=1):
    ds = d if isinstance(d, (tuple, list)) else (d,) * (len(bonds) - 1)
    return [[bonds[i], ds[i], danc, bonds[i + 1]] for i in range(len(bonds) - 1)]


def test_header_binding_and_library_agree():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "mpsengine.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(E.LIB_PATH)
    for name in NAMES:
        assert f"int {name}(" in header and name in E.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert E.Engine.RDM2_STATS == ("chain_kernel", "enqueued", "sites", "pairs")


def test_plan_reports_its_limits():
    ok, info = mps_rdm2_plan(_table((1, 4, 4, 1)), (0, 2), True)
    assert tuple(info) == RDM2_PLAN_INFO and RDM2_PLAN_INFO[:12] == RDM1_PLAN_INFO and info["valid"] == 1
    assert RDM2_PLAN_INFO[12:] == ("units", "out_elems", "stack_bytes")
    # entries 0 to 11 mean what they mean for mpse_mps_rdm1_plan; the limit of the rule is this call's own
    one = mps_rdm1_plan(_table((1, 4, 4, 1)), 2, True)[1]
    assert all(info[k] == one[k] for k in RDM1_PLAN_INFO if k not in ("bond_limit", "lds_bytes"))
    assert 1 <= info["bond_limit"] <= info["bond_fit_limit"]
    # by hand: E = 4 rows of pitch 5, T = 4 rows of pitch 5, complex: (20 + 20) * 16 = 640 bytes; real: 320
    assert info["e_elems"] == 20 and info["t_elems"] == 20 and info["lds_fit_bytes"] == 640
    assert ok == (info["bond_limit"] >= 4) and info["lds_bytes"] == (640 if ok else 0) and info["max_bond"] == 4
    assert info["units"] == 4 and info["out_elems"] == 16           # one opening site of d = 2, one pair
    assert info["stack_bytes"] == 256 << 20
    ok_r, real = mps_rdm2_plan(_table((1, 4, 4, 1)), (0, 2), False)
    assert real["lds_fit_bytes"] == 320 and ok_r == ok


def test_units_and_result_size_by_hand():
    """bonds (1, 2, 6, 1), d = (2, 3, 2), all three sites: units 4 + 9 = 13, result 4*9 + 4*4 + 9*4 = 88; E = 6 * 7,
    T = max(1 * 3, 2 * 7, 6 * 1)"""
    tab = _table((1, 2, 6, 1), d=(2, 3, 2))
    info = mps_rdm2_plan(tab, (0, 1, 2), True)[1]
    assert info["units"] == 13 and info["out_elems"] == 88
    assert info["e_elems"] == 42 and info["t_elems"] == 14 and info["lds_fit_bytes"] == 56 * 16
    # the last selected site opens nothing, the first closes nothing
    assert mps_rdm2_plan(tab, (0, 2), True)[1]["units"] == 4 and mps_rdm2_plan(tab, (0, 2), True)[1]["out_elems"] == 16
    assert mps_rdm2_plan(tab, (1, 2), True)[1]["units"] == 9 and mps_rdm2_plan(tab, (1, 2), True)[1]["out_elems"] == 36
    assert mps_rdm2_plan(tab, (0, 1), False)[1]["units"] == 4 and mps_rdm2_plan(tab, (0, 1), False)[1]["out_elems"] == 36


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(cplx):
    sel = (0, 1, 3)
    limit = mps_rdm2_plan(_table((1, 1, 1)), (0, 1), cplx)[1]["bond_limit"]
    ok, info = mps_rdm2_plan(_table((1, limit, limit, limit, 1)), sel, cplx)
    assert ok and info["max_bond"] == limit
    assert info["e_elems"] == limit * (limit | 1) and info["t_elems"] == limit * (limit | 1)
    assert 0 < info["lds_bytes"] <= info["lds_budget"]
    ok, info = mps_rdm2_plan(_table((1, limit, limit + 1, limit, 1)), sel, cplx)
    assert not ok and info["valid"] == 1 and info["lds_bytes"] == 0 and info["max_bond"] == limit + 1
    assert info["units"] == 8 and info["out_elems"] == 3 * 16       # the sizes do not depend on the path
    # what the LDS allows is a second, wider limit: launches up to it fit (MPSE_RDM2_CHAIN=1 runs them), none above
    fit = info["bond_fit_limit"]
    assert (info["lds_fit_bytes"] > 0) == (limit + 1 <= fit)
    ok, info = mps_rdm2_plan(_table((1, fit, fit, fit, 1)), sel, cplx)
    assert ok == (fit <= limit) and info["lds_fit_bytes"] == 2 * fit * (fit + 1) * (16 if cplx else 8)
    assert info["lds_fit_bytes"] <= info["lds_budget"] and info["e_elems"] == fit * (fit + 1)
    ok, info = mps_rdm2_plan(_table((1, fit, fit + 1, fit, 1)), sel, cplx)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["e_elems"] == 0


def test_offsets_stay_inside_32_bits():
    """the pooled environments (L_k: D_l^2, G_l: d_l^2 D_l^2 elements) and the result each stay below 2^31 elements"""
    # two sites of d = 128 and bond 1: the result 128^4 = 2^28 fits; d = 256: 2^32 does not
    assert mps_rdm2_plan(_table((1, 1, 1), d=128), (0, 1), False)[1]["lds_fit_bytes"] > 0
    ok, info = mps_rdm2_plan(_table((1, 1, 1), d=256), (0, 1), False)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["out_elems"] == 2 ** 32
    # d = 1024 behind a bond of 64: G alone holds 2^20 * 2^12 = 2^32 elements, the result only 4 * 2^20
    tab = [[1, 2, 1, 64], [64, 1024, 1, 1]]
    ok, info = mps_rdm2_plan(tab, (0, 1), False)
    assert not ok and info["lds_fit_bytes"] == 0 and info["out_elems"] == 4 * 2 ** 20
    assert mps_rdm2_plan([[1, 2, 1, 16], [16, 1024, 1, 1]], (0, 1), False)[1]["lds_fit_bytes"] > 0


def test_physical_extent_over_the_limit():
    for d, danc in ((65537, 1), (256, 257), (1, 65537)):
        ok, info = mps_rdm2_plan(_table((1, 1, 1), d=d, danc=danc), (0, 1), False)
        assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0
    assert mps_rdm2_plan(_table((1, 1, 1), d=1, danc=65536), (0, 1), False)[0]


def test_tables_that_are_no_chain():
    good = _table((1, 1, 1, 1))
    assert mps_rdm2_plan(good, (0, 2), True)[0]
    for i, j, v in ((0, 0, 2), (2, 3, 2), (1, 0, 4), (1, 1, 0), (1, 2, 0), (2, 3, -1)):
        bad = [list(r) for r in good]
        bad[i][j] = v
        ok, info = mps_rdm2_plan(bad, (0, 2), True)
        assert not ok and info["valid"] == 0 and info["max_bond"] == 0 and info["units"] == 0, bad
    assert not mps_rdm2_plan([], (0, 1), True)[0] and mps_rdm2_plan([], (0, 1), True)[1]["valid"] == 0


def test_fewer_than_two_sites_and_bad_selections():
    tab = _table((1,) * 303)                          # 302 sites
    ok, info = mps_rdm2_plan(tab, tuple(range(300)), True)
    assert ok and info["units"] == 4 * 299 and info["out_elems"] == 16 * 300 * 299 // 2
    for sel in ((), (5,)):                            # no pair: refused, the table itself is a chain
        ok, info = mps_rdm2_plan(tab, sel, True)
        assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["out_elems"] == 0
    for sel in ((2, 0), (1, 1), (0, 302), (-1, 1)):   # descending, duplicated, out of range
        ok, info = mps_rdm2_plan(tab, sel, True)
        assert not ok and info["valid"] == 1 and info["units"] == 0 and info["out_elems"] == 0


def test_selection_is_checked_before_the_library():
    """``Engine.mps_rdm2`` refuses through ``check_selection`` and a count of its own; neither needs a context"""
    assert check_selection("mps_rdm2", (0, 2, 5), 6) == [0, 2, 5]
    for sel, n in (((2, 0), 3), ((1, 1), 3), ((0, 3), 3), ((-1, 1), 3), ((), 3)):
        with pytest.raises(ValueError):
            check_selection("mps_rdm2", sel, n)

    class Site:
        ndim, shape = 3, (1, 2, 1)

    stub = E.Engine.__new__(E.Engine)                 # no context: the checks come before the library
    for sel in ((1,), (), (1, 0), (0, 3)):
        with pytest.raises(ValueError):
            E.Engine.mps_rdm2(stub, [Site(), Site(), Site()], sel)
