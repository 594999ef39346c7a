"""CPU checks of the integer rules of the asynchronous Lanczos solve (renormalizer_amd/csrc/mpse_lanczos_plan.h,
compiled by g++ through tests/host_emu/lanczos_plan_emu.cpp): the schedule that a single solve and the members of a
batch share, and the layout of a member's region of the slab."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINTS = (0, 7, 20, 63)
MAX_DIMS = (8, 20, 63, 64, 100, 128)         # limits 8, 20, 63 and 64 (one wavefront of coefficients)
SECTIONS = ("scal", "flag", "dot", "norm0", "norm1", "parts", "spare", "basis")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_lanczos_plan") / "liblanczos_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "lanczos_plan_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_schedule.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.emu_step.argtypes = [C.c_int] * 4
    lib.emu_layout.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.emu_constants.argtypes = [C.POINTER(C.c_int)]
    return lib


def _schedule(emu, hint, max_dim):
    out = (C.c_int * 4)()
    emu.emu_schedule(hint, max_dim, out)
    return dict(zip(("limit", "wait_from", "cap", "grown"), out))


def _layout(emu, n, cplx, parts, dot_cap, cap):
    out = (C.c_longlong * 11)()
    emu.emu_layout(n, int(cplx), parts, dot_cap, cap, out)
    return dict(zip(SECTIONS + ("stride", "ctl", "coef"), out))


def _constants(emu):
    out = (C.c_int * 5)()
    emu.emu_constants(out)
    return dict(zip(("maxm", "dot_cap", "norm_cap", "scalars", "ctl_doubles"), out))


@pytest.mark.parametrize("hint,max_dim", list(itertools.product(HINTS, MAX_DIMS)))
def test_schedule_numbers(emu, hint, max_dim):
    s = _schedule(emu, hint, max_dim)
    limit = min(max_dim, 64)
    assert s["limit"] == limit
    assert s["wait_from"] == max(hint - 1, 6)
    assert s["cap"] == min(max(hint + 4, 16), limit + 1)
    assert s["grown"] == min(2 * s["cap"], limit + 1)
    # the basis holds U_0 .. U_limit at the most, and growing reaches that: cap -> 2 cap -> .. -> limit + 1
    cap, steps = s["cap"], 0
    while cap < limit + 1:
        cap, steps = min(2 * cap, limit + 1), steps + 1
    assert steps <= 3


@pytest.mark.parametrize("hint,max_dim", list(itertools.product(HINTS, MAX_DIMS)))
def test_schedule_steps(emu, hint, max_dim):
    limit = min(max_dim, 64)
    for have_prev, j in itertools.product((0, 1), range(0, 70)):
        bits = emu.emu_step(hint, max_dim, j, have_prev)
        check, last, merged = bool(bits & 1), bool(bits & 2), bool(bits & 4)
        want = j > 3 and j % 2 == 0
        if j == 4 and not have_prev and j + 3 < limit:
            want = False                         # evaluated together with the check at j = 6
        assert check == want, (j, have_prev)
        assert last == (j + 1 >= limit), (j, have_prev)
        assert merged == (j == 6 and not have_prev), (j, have_prev)
        assert not merged or check


def test_first_check_of_a_solve(emu):
    """without an earlier estimate: limits up to 7 keep their check at j = 4 (there is no j = 6 to merge it into, or it
    would be the last); from 8 on the first check is the merged one at j = 6"""
    for limit in range(5, 12):
        first = next(j for j in range(limit) if emu.emu_step(0, limit, j, 0) & 1)
        assert first == (4 if limit <= 7 else 6), limit
        assert bool(emu.emu_step(0, limit, first, 0) & 4) == (first == 6)


SIZES = (258, 360, 2040, 257, 2049)          # (257 and 2049: sizes one double above a 256-byte boundary)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("parts", [1, 2, 4])
@pytest.mark.parametrize("n", SIZES)
def test_layout_sections(emu, n, parts, cplx):
    k = _constants(emu)
    nd = n * (2 if cplx else 1)
    for dot_cap, cap in itertools.product((8, 31, k["dot_cap"]), (2, 9, 16, 17, 24, 32, 33, 64, 65)):
        lay = _layout(emu, n, cplx, parts, dot_cap, cap)
        offs = [lay[s] for s in SECTIONS] + [lay["stride"]]
        assert offs[0] == 0 and all(o % 32 == 0 for o in offs), lay        # 256-byte boundaries (and strides)
        need = {"scal": k["scalars"] + 8 + 4 * k["maxm"], "flag": 1, "dot": 2 * dot_cap, "norm0": 2 * k["norm_cap"],
                "norm1": 2 * k["norm_cap"], "parts": parts * nd, "spare": nd, "basis": cap * nd}
        for s, lo, hi in zip(SECTIONS, offs[:-1], offs[1:]):               # in order, disjoint, each long enough
            assert hi - lo >= need[s], (s, lay)
            assert hi - lo < need[s] + 32, (s, lay)                        # (and nothing wasted beyond the alignment)
        # inside the first section: scalars, then the control block, then four rows of coefficients
        assert lay["ctl"] == k["scalars"] and lay["coef"] >= lay["ctl"] + k["ctl_doubles"]
        assert lay["flag"] - lay["coef"] >= 4 * k["maxm"]


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", SIZES)
def test_layout_growth(emu, n, cplx):
    """growing the basis moves no section in front of it, and the new stride covers the grown basis"""
    k = _constants(emu)
    nd = n * (2 if cplx else 1)
    for hint, max_dim, parts in itertools.product(HINTS, MAX_DIMS, (1, 2, 4)):
        s = _schedule(emu, hint, max_dim)
        a = _layout(emu, n, cplx, parts, k["dot_cap"], s["cap"])
        b = _layout(emu, n, cplx, parts, k["dot_cap"], s["grown"])
        assert all(a[x] == b[x] for x in SECTIONS + ("ctl", "coef")), (a, b)
        assert b["stride"] - b["basis"] >= s["grown"] * nd and b["stride"] >= a["stride"]
