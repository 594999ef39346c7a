"""CPU checks of the plan store's host side (renormalizer_amd/csrc/mpse_plan_store.h, compiled by g++ through
tests/host_emu/plan_store_emu.cpp): lookup, least-recently-used eviction under a byte budget, borrowed slots, and the
rule that decides on the host whether a slot's fused-matvec plan may be re-used."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH, SHAPE, TERMS, HIT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_plan_store") / "libplan_store_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "plan_store_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_reset.argtypes = [C.c_longlong]
    lib.emu_find.argtypes = [C.c_longlong]
    lib.emu_put.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int]
    lib.emu_release.argtypes = [C.c_longlong]
    lib.emu_total.restype = C.c_longlong
    lib.emu_released.argtypes = [C.POINTER(C.c_int), C.c_int]
    lib.emu_f0_match.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return lib


def _released(emu):
    buf = (C.c_int * 64)()
    n = emu.emu_released(buf, 64)
    return list(buf[:n])


def test_lookup_and_charge(emu):
    emu.emu_reset(1000)
    assert emu.emu_find(7) == 0 and emu.emu_count() == 0
    assert emu.emu_put(7, 300, 70, 0) == 0 and emu.emu_put(8, 300, 80, 0) == 0
    assert emu.emu_find(7) == 1 and emu.emu_find(8) == 1 and emu.emu_find(9) == 0
    assert emu.emu_total() == 600 and emu.emu_count() == 2
    assert emu.emu_put(7, 500, 71, 0) == 0          # the same key again: its bytes are replaced, not added
    assert emu.emu_total() == 800 and emu.emu_count() == 2 and _released(emu) == []


def test_lru_under_budget(emu):
    emu.emu_reset(1000)
    for k in (1, 2, 3):
        assert emu.emu_put(k, 300, 10 * k, 0) == 0
    assert emu.emu_find(1) == 1                      # 1 is now the most recently used, 2 the least
    assert emu.emu_put(4, 300, 40, 0) == 1 and _released(emu) == [20]
    assert emu.emu_find(2) == 0 and emu.emu_total() == 900
    assert emu.emu_put(5, 700, 50, 0) == 2 and _released(emu) == [20, 30, 10]     # 3, then 1 (4 is younger)
    assert emu.emu_total() == 1000 and emu.emu_count() == 2
    # a slot larger than the budget: everything else goes, then -1 and the slot owns nothing
    assert emu.emu_put(6, 1001, 60, 0) == -1 and emu.emu_last_evicted() == 2      # (counted although no room was found)
    assert emu.emu_total() == 0 and emu.emu_find(6) == 1 and sorted(_released(emu)) == [10, 20, 30, 40, 50]


def test_borrowed_slots_stay(emu):
    emu.emu_reset(1000)
    assert emu.emu_put(1, 400, 10, 1) == 0 and emu.emu_put(2, 400, 20, 0) == 0
    assert emu.emu_put(3, 400, 30, 0) == 1 and _released(emu) == [20]            # 1 is older but borrowed
    assert emu.emu_put(4, 400, 40, 0) == 1 and _released(emu) == [20, 30]
    assert emu.emu_put(5, 700, 50, 0) == -1 and emu.emu_find(1) == 1             # 4 went, 1 cannot: no room
    assert emu.emu_last_evicted() == 1
    emu.emu_release(1)
    assert emu.emu_put(5, 700, 50, 0) == 1 and emu.emu_find(1) == 0 and emu.emu_total() == 700


def test_f0_match_rules(emu):
    sig = np.array([256, 256, 5, 5, 2, 1, 256, 1, 16, 128, 1], dtype=np.int32)
    terms = bytes(range(200))

    def match(have, kept, kt, now, nt):
        return emu.emu_f0_match(have, kept.ctypes.data_as(C.POINTER(C.c_int)), kt, len(kt),
                                now.ctypes.data_as(C.POINTER(C.c_int)), nt, len(nt))

    assert match(0, sig, terms, sig, terms) == FRESH
    assert match(1, sig, terms, sig, terms) == HIT
    for i in range(len(sig)):                        # every field of the signature counts
        other = sig.copy()
        other[i] += 1
        assert match(1, sig, terms, other, terms) == SHAPE, i
    flipped = bytearray(terms)
    flipped[137] ^= 1
    assert match(1, sig, terms, sig, bytes(flipped)) == TERMS
    assert match(1, sig, terms, sig, terms[:-8]) == TERMS
    assert match(1, sig, b"", sig, b"") == HIT
