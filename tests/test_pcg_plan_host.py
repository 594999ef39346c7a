"""CPU checks of the integer rules of the conjugate-gradient solver (renormalizer_amd/csrc/mpse_pcg_plan.h, compiled by
g++ through tests/host_emu/pcg_plan_emu.cpp): when the host waits for the decision, the default iteration limit, and
the layout of a member's region of the slab, which a single solve, a summed solve and the members of a batch share."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ("ctl", "part_bb", "part_bx", "part_rz0", "part_rz1", "part_pq", "y", "q", "r", "p", "extra_y")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_pcg_plan") / "libpcg_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "pcg_plan_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_waits_at.argtypes = [C.c_int, C.c_int]
    lib.emu_default_max_iter.argtypes = [C.c_longlong]
    lib.emu_layout.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.emu_constants.argtypes = [C.POINTER(C.c_int)]
    return lib


def _constants(emu):
    out = (C.c_int * 2)()
    emu.emu_constants(out)
    return dict(zip(("k", "cw"), out))


def _layout(emu, n, cplx, nb, nbq, extra_y):
    out = (C.c_longlong * 14)()
    emu.emu_layout(n, int(cplx), nb, nbq, extra_y, out)
    return dict(zip(SECTIONS + ("end", "stride", "vec"), out))


@pytest.mark.parametrize("max_iter", [1, 3, 4, 5, 8])
def test_waits(emu, max_iter):
    K = _constants(emu)["k"]
    assert K == 4
    waits = [k for k in range(max_iter + 1) if emu.emu_waits_at(k, max_iter)]
    # every K-th iteration, and the limit itself: the kernel decides at k == max_iter at the latest
    assert waits == sorted(set(range(K - 1, max_iter + 1, K)) | {max_iter})
    # whichever iteration the decision falls at, the host reads it at most K - 1 iterations later
    for decided in range(max_iter + 1):
        first = next(k for k in range(decided, max_iter + 1) if emu.emu_waits_at(k, max_iter))
        assert first - decided <= K - 1, (decided, first)


def test_default_max_iter(emu):
    assert emu.emu_default_max_iter(1) == 10
    assert emu.emu_default_max_iter(65536) == 655360
    assert emu.emu_default_max_iter(2 ** 27) == 10 * 2 ** 27          # (the last that fits an int)
    assert emu.emu_default_max_iter(2 ** 27 + 1) == 2 ** 30


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 257, 7735])
def test_layout_sections(emu, n, cplx):
    cw = _constants(emu)["cw"]
    es = 16 if cplx else 8
    for nb, extra_y in itertools.product((1, 2, 512), (0, 2, 3)):
        for nbq in sorted({nb, 1, 64}):
            lay = _layout(emu, n, cplx, nb, nbq, extra_y)
            offs = [lay[s] for s in SECTIONS] + [lay["end"]]
            assert offs[0] == 0 and all(o % 256 == 0 for o in offs), lay
            pairs = 2 * nb * 8
            need = {"ctl": cw * 8, "part_bb": pairs, "part_bx": pairs, "part_rz0": pairs, "part_rz1": pairs,
                    "part_pq": 2 * max(nb, nbq) * 8, "y": n * es, "q": n * es, "r": n * es, "p": n * es,
                    "extra_y": extra_y * n * es}
            for s, lo, hi in zip(SECTIONS, offs[:-1], offs[1:]):           # in order, disjoint, each long enough
                assert hi - lo >= need[s], (s, lay)
            for s in SECTIONS[:-1]:                                        # (and nothing wasted beyond the alignment)
                assert lay[SECTIONS[SECTIONS.index(s) + 1]] - lay[s] < need[s] + 256, (s, lay)
            # the further y vectors: whole aligned vectors, one vector apart
            assert lay["vec"] % 256 == 0 and lay["vec"] >= n * es
            assert lay["end"] - lay["extra_y"] == extra_y * lay["vec"]
            assert lay["q"] - lay["y"] == lay["vec"]
            assert lay["stride"] >= lay["end"] and lay["stride"] % 256 == 0
