"""Host side of the one-site density matrices (no GPU): the path rule of ``mpse_mps_rdm1_plan`` on dims tables and the
checks ``Engine.mps_rdm1`` makes before it calls the library.

LDS plan of either launch (renormalizer_amd/csrc/mpse_rdm1.hip): region E, the largest D * (D | 1) over the bonds, plus
region T, the largest D_l * (D_r | 1) over the sites, in working elements of 8 (real) or 16 (complex) bytes; no reduction
words, the sums of ``k_rdm1_sites`` go through lane shuffles."""
import pytest

from renormalizer_amd.engine import RDM1_PLAN_INFO, check_selection, mps_rdm1_plan


def _table(bonds, d=2, danc=1):
    return [[bonds[i], d, danc, bonds[i + 1]] for i in range(len(bonds) - 1)]


def test_plan_reports_its_limits():
    ok, info = mps_rdm1_plan(_table((1, 4, 4, 1)), 2, True)
    assert tuple(info) == RDM1_PLAN_INFO and info["valid"] == 1
    assert info["lds_budget"] == 160 * 1024 and info["threads"] == 1024
    assert 1 <= info["bond_limit"] <= info["bond_fit_limit"]              # the rule's limit is a measured one
    fit = info["bond_fit_limit"]
    # the fit limit is the largest power of two whose two padded complex regions lie inside the budget
    assert fit & (fit - 1) == 0 and 2 * fit * (fit + 1) * 16 <= info["lds_budget"] < 2 * 2 * fit * (2 * fit + 1) * 16
    assert info["nsel_limit"] == 0 and info["p_limit"] == 65536           # no cap on the selection
    # by hand: E = 4 rows of pitch 5, T = 4 rows of pitch 5, complex: (20 + 20) * 16 = 640 bytes; real: 320
    assert info["e_elems"] == 20 and info["t_elems"] == 20 and info["lds_fit_bytes"] == 640
    assert ok == (info["bond_limit"] >= 4) and info["lds_bytes"] == (640 if ok else 0)
    assert info["max_bond"] == 4
    ok_r, real = mps_rdm1_plan(_table((1, 4, 4, 1)), 2, False)
    assert real["lds_fit_bytes"] == 320 and real["lds_bytes"] == (320 if ok_r else 0) and ok_r == ok
    # T follows D_l * pitch(D_r) of a site, E the largest square: bonds (1, 2, 6, 1): E = 6 * 7, T = max(1 * 3, 2 * 7, 6 * 1)
    info = mps_rdm1_plan(_table((1, 2, 6, 1)), 1, True)[1]
    assert info["e_elems"] == 42 and info["t_elems"] == 14 and info["lds_fit_bytes"] == 56 * 16


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(cplx):
    limit = mps_rdm1_plan(_table((1, 1)), 1, cplx)[1]["bond_limit"]
    ok, info = mps_rdm1_plan(_table((1, limit, limit, limit, 1)), 3, cplx)
    assert ok and info["max_bond"] == limit
    assert info["e_elems"] == limit * (limit | 1) and info["t_elems"] == limit * (limit | 1)
    assert 0 < info["lds_bytes"] <= info["lds_budget"]
    ok, info = mps_rdm1_plan(_table((1, limit, limit + 1, limit, 1)), 3, cplx)
    assert not ok and info["valid"] == 1 and info["lds_bytes"] == 0 and info["max_bond"] == limit + 1
    # what the LDS allows is a second, wider limit: launches up to it fit (MPSE_RDM1_CHAIN=1 runs them), none above
    fit = info["bond_fit_limit"]
    assert (info["lds_fit_bytes"] > 0) == (limit + 1 <= fit)
    ok, info = mps_rdm1_plan(_table((1, fit, fit, fit, 1)), 3, cplx)
    assert ok == (fit <= limit) and info["lds_fit_bytes"] == 2 * fit * (fit + 1) * (16 if cplx else 8)
    assert info["lds_fit_bytes"] <= info["lds_budget"] and info["e_elems"] == fit * (fit + 1)
    ok, info = mps_rdm1_plan(_table((1, fit, fit + 1, fit, 1)), 3, cplx)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["e_elems"] == 0


def test_physical_extent_over_the_limit():
    assert mps_rdm1_plan(_table((1, 1, 1), d=65536), 1, False)[0]
    assert mps_rdm1_plan(_table((1, 1, 1), d=256, danc=256), 1, False)[0]
    for d, danc in ((65537, 1), (256, 257), (1, 65537)):
        ok, info = mps_rdm1_plan(_table((1, 1, 1), d=d, danc=danc), 1, False)
        assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0


def test_tables_that_are_no_chain():
    good = _table((1, 1, 1, 1))
    assert mps_rdm1_plan(good, 2, True)[0]
    for i, j, v in ((0, 0, 2), (2, 3, 2), (1, 0, 4), (1, 1, 0), (1, 2, 0), (2, 3, -1)):
        bad = [list(r) for r in good]
        bad[i][j] = v
        ok, info = mps_rdm1_plan(bad, 2, True)
        assert not ok and info["valid"] == 0 and info["max_bond"] == 0, bad
    assert not mps_rdm1_plan([], 1, True)[0] and mps_rdm1_plan([], 1, True)[1]["valid"] == 0


def test_any_number_of_selected_sites():
    tab = _table((1,) + (1,) * 301 + (1,))          # 302 sites
    assert len(tab) == 302
    ok, info = mps_rdm1_plan(tab, 300, True)
    assert ok and info["lds_fit_bytes"] == 2 * 16
    ok, info = mps_rdm1_plan(tab, 0, True)           # an empty selection is refused
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0
    assert not mps_rdm1_plan(tab, -1, True)[0]


def test_selection_is_checked_before_the_library():
    assert check_selection("mps_rdm1", (0, 2, 5), 6) == [0, 2, 5]
    assert check_selection("mps_rdm1", [3], 4) == [3]
    for sel, n in (((2, 0), 3), ((1, 1), 3), ((0, 3), 3), ((-1, 1), 3), ((), 3), ((0, 2, 1), 3)):
        with pytest.raises(ValueError):
            check_selection("mps_rdm1", sel, n)
