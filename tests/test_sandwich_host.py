"""Host side of ``mpse_mps_sandwich``: the symbols exist where they are declared, and ``mpse_mps_sandwich_plan`` - the
path rule on the dims table alone - reports what the table implies.  Needs the built library, no GPU.  Every limit
(LDS budget, accumulators, work bound) is read from the plan's ``info``, none is written here as a literal except the
160 KiB of a gfx950 compute unit."""
import os

from renormalizer_amd import engine
from renormalizer_amd.engine import mps_sandwich_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpse_mps_sandwich", "mpse_mps_sandwich_plan", "mpse_mps_sandwich_stats")


def _rows(bra, ket, w, d, danc=1):
    """dims rows of a chain from its bond lists; d / danc: one value or one per site"""
    n = len(bra) - 1
    ds = [d] * n if isinstance(d, int) else list(d)
    das = [danc] * n if isinstance(danc, int) else list(danc)
    return [[bra[i], ket[i], w[i], ds[i], das[i], bra[i + 1], ket[i + 1], w[i + 1]] for i in range(n)]


def _pitch(k):
    return k | 1


def _implied_elems(rows):
    """(elements of E, elements of T) as the header states them: E = Db * w rows of Dk elements padded to an odd
    length, the largest over all bonds; T = Db_l * wl * Dk_r, the largest over the sites"""
    e = max(max(r[0] * r[2] * _pitch(r[1]), r[5] * r[7] * _pitch(r[6])) for r in rows)
    t = max(r[0] * r[2] * r[6] for r in rows)
    return e, t


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mpsengine.h")) as f:
        header = f.read()
    lib = engine.load_library()
    for name in NAMES:
        assert f"int {name}(" in header and name in engine.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert callable(engine.Engine.mps_sandwich) and callable(engine.Engine.mps_sandwich_stats)
    from renormalizer_amd.mps.mps import Mps
    from renormalizer_amd.mps.mpdm import MpDm
    assert callable(Mps.matrix_element) and MpDm.matrix_element is Mps.matrix_element
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "mpse_mps_sandwich" in f.read()


def test_budget_and_lds_bytes_follow_the_table():
    rows = _rows((1, 2, 5, 3, 2, 1), (1, 3, 4, 4, 3, 1), (1, 3, 5, 2, 4, 1), (2, 3, 2, 3, 2))
    for cplx in (False, True):
        ok, info = mps_sandwich_plan(rows, cplx)
        assert ok and info["valid"] == 1
        assert info["lds_budget"] == 160 * 1024
        assert info["elem_bytes"] == (16 if cplx else 8)
        assert (info["e_elems"], info["t_elems"]) == _implied_elems(rows)
        assert info["lds_bytes"] == (info["e_elems"] + info["t_elems"]) * info["elem_bytes"]
        assert 0 < info["lds_bytes"] <= info["lds_budget"]
        assert info["acc_needed"] <= info["acc_per_thread"] and 0 < info["work"] <= info["work_max"]
    # the work of the heaviest site: d danc (Dbl wl Dkl Dkr + d wl Dbl Dbr Dkr)
    assert info["work"] == max(r[3] * r[4] * (r[0] * r[2] * r[1] * r[6] + r[3] * r[2] * r[0] * r[5] * r[6]) for r in rows)


def test_complex_needs_at_least_the_bytes_of_real():
    rows = _rows((1, 8, 16, 8, 1), (1, 6, 12, 6, 1), (1, 4, 4, 4, 1), 2, 2)
    (ok_r, real), (ok_c, cplx) = mps_sandwich_plan(rows, False), mps_sandwich_plan(rows, True)
    assert ok_r and ok_c and cplx["lds_bytes"] == 2 * real["lds_bytes"] >= real["lds_bytes"]
    # a chain whose real launch fits and whose complex launch does not
    big = _rows((1, 40, 40, 1), (1, 41, 41, 1), (1, 4, 4, 1), 2)
    assert mps_sandwich_plan(big, False)[0] and not mps_sandwich_plan(big, True)[0]


def test_eligibility_is_monotone():
    """growing a bond, an MPO bond or d * danc never turns an ineligible chain eligible and never shrinks the launch of
    an eligible one"""
    def grown(base, which, k):
        bra, ket, w, d, danc = [list(x) if isinstance(x, tuple) else x for x in base]
        if which == "bra":
            bra[2] += k
        elif which == "ket":
            ket[2] += k
        elif which == "w":
            w[2] += k
        elif which == "d":
            d += k
        else:
            danc += k
        return _rows(bra, ket, w, d, danc)

    bases = [((1, 6, 20, 6, 1), (1, 5, 24, 5, 1), (1, 3, 3, 3, 1), 2, 2),
             ((1, 8, 30, 8, 1), (1, 8, 30, 8, 1), (1, 4, 5, 4, 1), 4, 1),
             ((1, 2, 2, 2, 1), (1, 2, 2, 2, 1), (1, 1, 1, 1, 1), 3, 3)]
    steps = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 400, 1500, 70000)
    for base in bases:
        for cplx in (False, True):
            for which in ("bra", "ket", "w", "d", "danc"):
                was_ok, was_lds, was_work = True, 0, 0
                for k in (0,) + steps:
                    ok, info = mps_sandwich_plan(grown(base, which, k), cplx)
                    assert info["valid"] == 1
                    assert not (ok and not was_ok), (base, which, k)
                    if ok:
                        assert info["lds_bytes"] >= was_lds, (base, which, k)
                        was_lds = info["lds_bytes"]
                    else:
                        assert info["lds_bytes"] == 0
                    assert info["work"] >= was_work
                    was_ok, was_work = ok, info["work"]
                assert not was_ok, (base, which)      # the last step is beyond every limit


def _limit_chain(extra_channels=0):
    """a complex two-site chain whose launch is exactly the LDS budget: one inner bond (a, k, w) with k odd (no
    padding), E = a w k and T = a w (the second site's), so a w (k + 1) * 16 bytes = budget; nearly no arithmetic"""
    budget = mps_sandwich_plan([[1] * 8], True)[1]["lds_budget"]
    k, w = 3, 5
    a, rest = divmod(budget, 16 * w * (k + 1))
    assert rest == 0
    return _rows((1, a, 1), (1, k, 1), (1, w + extra_channels, 1), 2), budget


def test_exactly_at_the_lds_limit_and_one_channel_more():
    rows, budget = _limit_chain()
    ok, info = mps_sandwich_plan(rows, True)
    assert ok and info["lds_bytes"] == budget == info["lds_budget"], info
    assert info["acc_needed"] <= info["acc_per_thread"] and info["work"] <= info["work_max"]
    rows1, _ = _limit_chain(1)
    ok1, info1 = mps_sandwich_plan(rows1, True)
    assert not ok1 and info1["valid"] == 1 and info1["lds_bytes"] == 0
    # it is the LDS that refuses the twin: accumulators, channels and work are within their limits
    assert (info1["e_elems"] + info1["t_elems"]) * info1["elem_bytes"] > budget
    assert info1["acc_needed"] <= info1["acc_per_thread"] and info1["work"] <= info1["work_max"]
    assert max(r[7] for r in rows1) <= info1["channel_limit"]


def test_over_the_work_bound_is_refused_although_it_fits():
    """d = danc grows on a chain of bond 8 until the heaviest site is over the work bound (read from the plan): up to
    the bound the chain is taken, beyond it it is not, although its LDS and its accumulators - which do not depend on
    the physical extents - still fit"""
    bonds, w = (1, 8, 8, 1), (1, 2, 2, 1)
    work_max = mps_sandwich_plan(_rows(bonds, bonds, w, 2, 2), False)[1]["work_max"]
    d, taken = 2, 0
    while True:      # work of the middle site = d^2 * 8^3 * 2 * (8 + d * 8) / 8
        rows = _rows(bonds, bonds, w, d, d)
        ok, info = mps_sandwich_plan(rows, False)
        assert info["valid"] == 1
        assert (info["e_elems"], info["t_elems"]) == _implied_elems(rows)
        if info["work"] > work_max:
            break
        taken += int(ok)
        d *= 2
        assert d <= 1 << 30, "no physical dimension reaches the work bound"
    assert taken >= 1
    assert not ok and info["lds_bytes"] == 0
    assert (info["e_elems"] + info["t_elems"]) * info["elem_bytes"] <= info["lds_budget"]
    assert info["acc_needed"] <= info["acc_per_thread"]
    # one step back the work is within the bound
    assert mps_sandwich_plan(_rows(bonds, bonds, w, d // 2, d // 2), False)[1]["work"] <= work_max


def test_tables_that_are_no_chain():
    good = _rows((1, 3, 1), (1, 2, 1), (1, 2, 1), 2)
    assert mps_sandwich_plan(good, False)[1]["valid"] == 1

    def bad(site, col, val):
        rows = [list(r) for r in good]
        rows[site][col] = val
        return rows

    cases = {"mismatched bra bond": bad(1, 0, 4), "mismatched ket bond": bad(0, 6, 3), "mismatched MPO bond": bad(1, 2, 3),
             "open first bond": bad(0, 0, 2), "open last ket bond": bad(1, 6, 2), "open first MPO bond": bad(0, 2, 2),
             "open last MPO bond": bad(1, 7, 2), "extent 0": bad(0, 3, 0), "ancilla 0": bad(1, 4, 0), "no sites": []}
    for name, rows in cases.items():
        for cplx in (False, True):
            ok, info = mps_sandwich_plan(rows, cplx)
            assert not ok and info["valid"] == 0 and info["lds_bytes"] == 0, name
