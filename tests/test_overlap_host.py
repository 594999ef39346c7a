"""The path rule of ``mpse_mps_overlap`` on the shape alone (``mpse_mps_overlap_plan``: no context, no GPU), and the
new symbols of the C header."""
import itertools
import os
import re

from renormalizer_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(bra_bonds, ket_bonds, p=2):
    return [[bra_bonds[i], ket_bonds[i], p, bra_bonds[i + 1], ket_bonds[i + 1]] for i in range(len(bra_bonds) - 1)]


def test_limit_is_derived_from_the_lds_budget():
    _, info = E.mps_overlap_plan(_table((1, 1), (1, 1)), True)
    limit, budget = info["bond_limit"], info["lds_budget"]
    assert budget == 160 * 1024                       # LDS of a gfx950 compute unit
    assert limit & (limit - 1) == 0                   # a power of two
    # a complex E (rows padded to an odd length) and a T slice at the limit fit, at twice the limit they do not
    lds = lambda d: (d * (d | 1) + d * d) * 16
    assert lds(limit) <= budget < lds(2 * limit)
    # 64 x 64 complex128 twice is 128 KB: it leaves room for the padding
    assert limit == 64 and lds(64) == 132096


def test_eligible_at_the_limit_and_not_above():
    limit = E.mps_overlap_plan(_table((1, 1), (1, 1)), False)[1]["bond_limit"]
    for cplx in (False, True):
        at = _table((1, limit, limit, 1), (1, limit, limit, 1))
        ok, info = E.mps_overlap_plan(at, cplx)
        assert ok and info["max_bond"] == limit and 0 < info["lds_bytes"] <= info["lds_budget"]
        assert info["e_elems"] == limit * (limit | 1) and info["t_elems"] == limit * limit
        assert info["lds_bytes"] == (info["e_elems"] + info["t_elems"]) * (16 if cplx else 8)
        assert info["e_elems"] <= 4 * info["threads"] + limit      # one accumulator per entry of E (without padding)
        for side in (0, 1):
            bonds = [(1, limit, limit, 1), (1, limit, limit, 1)]
            bonds[side] = (1, limit + 1, limit, 1)
            ok, info = E.mps_overlap_plan(_table(*bonds), cplx)
            assert not ok and info["valid"] == 1 and info["lds_bytes"] == 0 and info["max_bond"] == limit + 1


def test_monotone_in_the_bonds_and_complex_needs_at_least_real():
    sizes = (1, 3, 17, 64, 65)
    prev = {}
    for db, dk in itertools.product(sizes, sizes):
        tab = _table((1, db, db, 1), (1, dk, dk, 1), p=3)
        ok_r, info_r = E.mps_overlap_plan(tab, False)
        ok_c, info_c = E.mps_overlap_plan(tab, True)
        assert ok_r == ok_c == (max(db, dk) <= 64)
        if ok_r:
            assert info_c["lds_bytes"] == 2 * info_r["lds_bytes"] >= info_r["lds_bytes"] > 0
        prev[(db, dk)] = (ok_r, info_r["lds_bytes"])
    for (db, dk), (ok, lds) in prev.items():
        for (db2, dk2), (ok2, lds2) in prev.items():
            if db2 >= db and dk2 >= dk:
                assert ok or not ok2                  # growing a bond never makes a chain eligible
                if ok2:
                    assert lds2 >= lds                # nor its launch smaller
    # the physical extent does not enter the LDS (sigma is walked), only the 32-bit offsets
    assert E.mps_overlap_plan(_table((1, 8, 1), (1, 8, 1), p=65536), True)[0]
    assert not E.mps_overlap_plan(_table((1, 8, 1), (1, 8, 1), p=65537), True)[0]


def test_tables_that_are_no_chain():
    for tab in ([[1, 1, 2, 3, 3], [4, 3, 2, 1, 1]], [[2, 1, 2, 3, 3], [3, 3, 2, 1, 1]], [[1, 1, 2, 3, 3], [3, 3, 2, 1, 2]],
                [[1, 1, 0, 1, 1]], []):
        ok, info = E.mps_overlap_plan(tab, False)
        assert not ok and info["valid"] == 0 and info["max_bond"] == 0 and info["lds_bytes"] == 0


def test_header_has_the_new_symbols():
    txt = open(os.path.join(REPO, "include", "mpsengine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = ("mpse_mps_overlap", "mpse_mps_overlap_stats", "mpse_mps_overlap_plan")
    for sym in names:
        assert re.search(rf"\bint {sym}\s*\(", code), sym
    assert set(names) <= set(E.EXPORTED_SYMBOLS)
    assert callable(E.Engine.mps_overlap) and callable(E.Engine.mps_overlap_stats)
