"""Host parts of the lock-step correction-vector run: the eligibility rule of the one-launch two-layer matvec and the
grouping of ``mpse_pcg_batch`` as pure functions, the refill order, and the new symbols of the C header."""
import collections
import os
import re

from renormalizer_amd.cv import lockstep as ls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eligibility_rule():
    ok = ls.small2_eligible
    assert ok(5, 3, 7, 3, 3, False) and ok(17, 4, 33, 5, 5, True)
    assert ok(24, 16, 24, 5, 5, False) and ok(24, 16, 24, 5, 5, True)          # the Holstein phonon site, both types
    assert ok(6, 3, 5, ls.SM2_WMAX, ls.SM2_WMAX, False) and not ok(6, 3, 5, ls.SM2_WMAX + 1, 3, False)
    assert not ok(6, 3, 5, 3, ls.SM2_WMAX + 1, False)
    assert ok(5, ls.SM2_DMAX, 4, 3, 3, True) and not ok(5, ls.SM2_DMAX + 1, 4, 3, 3, True)
    assert ok(ls.SM2_BMAX, 2, ls.SM2_BMAX, 3, 3, True) and not ok(ls.SM2_BMAX + 1, 2, 5, 3, 3, False)
    assert not ok(5, 2, ls.SM2_BMAX + 1, 3, 3, False) and not ok(0, 2, 5, 3, 3, False)
    # the LDS budget binds for complex centres at the widest MPO bond and physical dimension (sparse list 12.8 kB,
    # 2048 elements of intermediates per ket-bond state, 64 per row of L): (65536 - 256 - 12816) / 16 - 64 Dl >= 2048
    edge = max(v for v in range(1, ls.SM2_BMAX + 1) if ok(v, 16, 4, 8, 8, True))
    assert edge == 19 and all(ok(v, 16, 4, 8, 8, True) for v in range(1, edge)) and not ok(edge + 1, 16, 4, 8, 8, True)
    assert ok(ls.SM2_BMAX, 16, 4, 8, 8, False)
    # every plan stays inside the budget (+ the static words of the block reduction), slices and K groups >= 1
    for shp in ((5, 3, 7, 3, 3), (24, 16, 24, 5, 5), (64, 16, 64, 3, 3), (edge, 16, 4, 8, 8), (64, 2, 64, 8, 8)):
        for cplx in (False, True):
            plan = ls.small2_plan(*shp, cplx)
            if plan is not None:
                jh, g, lds = plan
                assert 1 <= jh <= shp[2] and 1 <= g <= 256 // shp[2] and lds + 256 <= ls.SM2_LDS_MAX
    # by hand: sparse list 128 doubles (5 + 41 + 81 + 1), row of L 45, intermediates 54 per state x 7 states, 36 K groups
    assert ls.small2_plan(5, 3, 7, 3, 3, False) == (7, 36, 8 * 128 + 8 * (45 + max(54 * 7, 36 * 3 * 7)))


def test_grouping():
    a, b, big = (5, 3, 7, 3, 3, False), (17, 4, 33, 5, 5, False), (5, 17, 4, 3, 3, False)
    sets, singles = ls.group_members([a, b, None, a, big, b], 32)
    assert sets == [[0, 3], [1, 5]] and singles == [2, 4]
    sets, singles = ls.group_members([a] * 5 + [b] + [a] * 2, 3)
    assert sets == [[0, 1, 2], [3, 4, 6], [7], [5]] and singles == []
    assert ls.group_members([], 4) == ([], [])
    # real and complex members of one shape do not share a set
    assert ls.group_members([a, a[:5] + (True,)], 4)[0] == [[0], [1]]


def test_refill_order():
    pending = collections.deque([3, 4, 5])
    assert ls.refill([0, 2], pending, 4) == [0, 2, 3, 4] and list(pending) == [5]
    assert ls.refill([0, 2, 3, 4], pending, 4) == [0, 2, 3, 4] and list(pending) == [5]
    assert ls.refill([], collections.deque(), 4) == []
    # members leave at different sweeps; the next frequency joins at the next sweep start, survivors keep their order
    rounds = ls.lockstep_schedule([2, 4, 3, 2, 1], 2)
    assert rounds == [[0, 1], [0, 1], [1, 2], [1, 2], [2, 3], [3, 4]]
    assert ls.lockstep_schedule([3, 1, 2], 8) == [[0, 1, 2], [0, 2], [0]]
    assert ls.lockstep_schedule([2, 2], 1) == [[0], [0], [1], [1]]


def test_header_has_the_new_symbols():
    txt = open(os.path.join(REPO, "include", "mpsengine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for sym in ("mpse_pcg_batch", "mpse_pcg_batch_stats", "mpse_pcg_batch_plan"):
        assert re.search(rf"\bint {sym}\s*\(", code), sym
    from renormalizer_amd import engine as E
    assert {"mpse_pcg_batch", "mpse_pcg_batch_stats", "mpse_pcg_batch_plan"} <= set(E.EXPORTED_SYMBOLS)
    assert callable(E.Engine.pcg_batch) and callable(E.Engine.pcg_batch_stats)
    from renormalizer_amd import cv
    assert callable(cv.batch_run_lockstep)
