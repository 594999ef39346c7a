"""CPU check of the integer rules of the contraction kernel (renormalizer_amd/csrc/mpse_gemm_tiles.h - what k_gemm of
mpse_gemm.hip calls between its loads and barriers), compiled with g++ from tests/host_emu/gemm_tiles_emu.cpp:
  * position map: for every plain and grouped launch plan on the boundary grids of tests/test_gemm_plan_host.py, and
    for hand-made halved launches, positions 0 .. nwg - 1 reach every (batch, K slice or half, group, tile row, tile
    column) exactly once - with and without a launch order, with dead tiles;
  * flag walk: next_flagged returns exactly the flagged K tiles of a range, in order, whatever lies beyond its end;
  * halved tiles: the two halves are disjoint, cover the occupied K tiles and hold n / 2 and n - n / 2 of them.
No GPU needed."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import test_gemm_plan_host as PH   # (the plan emulator's wrappers and the boundary grids)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path_factory, name, src):
    out = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(REPO, "tests", "host_emu", src), "-o", out])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    lib = _build(tmp_path_factory, "gemm_tiles_emu", "gemm_tiles_emu.cpp")
    lib.emu_positions_cover.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_longlong, C.POINTER(C.c_longlong)]
    lib.emu_launch_positions.argtypes = [C.POINTER(C.c_longlong), C.c_longlong, C.POINTER(C.c_int)]
    lib.emu_launch_positions.restype = None
    lib.emu_flag_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.emu_half_range.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.emu_half_range.restype = None
    lib.emu_tile_coords.argtypes = [C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.emu_tile_coords.restype = None
    lib.emu_next_flagged.argtypes = [C.c_void_p, C.c_int, C.c_int]
    return lib


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    lib = _build(tmp_path_factory, "plan_emu_for_tiles", "plan_emu.cpp")
    for fn in (lib.emu_gemm_launch_plan, lib.emu_gemm_grouped_plan):
        fn.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        fn.restype = None
    return lib


def _launch(tiles_m, tiles_n, batch=1, ksplit=1, slice_fast=0, die_group=0, skew=1, grouped=0, split2=0, cpd=32, tiles_m_grp=1):
    return (C.c_longlong * 11)(tiles_m, tiles_n, batch, ksplit, slice_fast, die_group, skew, grouped, split2, cpd, tiles_m_grp)


def _orders(ntile, grouped, rng):
    """launch orders to try: identity, reversed, shuffled; grouped launches also with dead marks (~tile)"""
    ident = list(range(ntile))
    shuffled = ident[:]
    rng.shuffle(shuffled)
    orders = [(ident, 0), (ident[::-1], 0), (shuffled, 0)]
    if grouped:
        dead = set(rng.sample(ident, ntile // 3))
        orders += [([~t if t in dead else t for t in shuffled], len(dead)), ([~t for t in ident], ntile)]
    return orders


def _cover(tiles, args, nwg, order=None, want_dead=0):
    perm = (C.c_int * len(order))(*order) if order is not None else None
    ndead = C.c_longlong(-1)
    rc = tiles.emu_positions_cover(args, perm, nwg, C.byref(ndead))
    assert rc == 0, ("check at line %d of gemm_tiles_emu.cpp" % rc, list(args), nwg, order is not None)
    rows = nwg // (args[0] * args[1])          # every dead tile is met once per K slice / half
    assert ndead.value == want_dead * rows


@pytest.mark.parametrize("n_cu", PH.N_CUS)
def test_plain_plans_map_positions_one_to_one(tiles, plans, n_cu):
    rng = random.Random(n_cu)
    seen = set()
    for (tm, tn, batch), nkt, hint in itertools.product(PH._tile_grids(n_cu), (1, 2, 3, 4, 5, 8, 9), (0, 3)):
        p = PH.c_plain(plans, n_cu, 64 * tm, 64 * tn, 16 * nkt, batch, 1, 1, hint)
        key = (p["tiles_m"], p["tiles_n"], batch, p["ksplit"], p["die_group"], p["order"])
        if key in seen:
            continue
        seen.add(key)
        args = _launch(p["tiles_m"], p["tiles_n"], batch, p["ksplit"], int(p["ksplit"] > 1 and batch == 1), p["die_group"])
        if p["order"]:
            for order, _ in _orders(p["tiles_m"] * p["tiles_n"], False, rng):
                _cover(tiles, args, p["nwg"], order)
        else:
            _cover(tiles, args, p["nwg"])
    kinds = {(k[3] > 1, k[4], k[5]) for k in seen}
    assert {(True, 0, 0), (False, 1, 0), (False, 2, 0), (False, 0, 0)} <= kinds       # split, die groups, skew ...
    assert n_cu < 64 or any(k[2] for k in kinds)                                        # ... and ordered launches


@pytest.mark.parametrize("n_cu", PH.N_CUS)
def test_grouped_plans_map_positions_one_to_one(tiles, plans, n_cu):
    rng = random.Random(1000 + n_cu)
    seen = set()
    for (tm, tn, _b), ngrp in itertools.product(PH._tile_grids(n_cu), (1, 2, 8)):
        if tm % ngrp:
            continue
        M, N = 64 * (tm // ngrp), 64 * tn
        for nkt_max, any_mask, split2 in itertools.product((8, 9), (0, 1), (0, 1)):
            split2 = int(split2 and ngrp == 1)
            p = PH.c_grouped(plans, n_cu, M, N, ngrp, nkt_max, any_mask, split2, 1)
            key = (p["tiles_m"], p["tiles_n"], ngrp, split2, p["die_group"], p["order"])
            if key in seen:
                continue
            seen.add(key)
            args = _launch(p["tiles_m"], p["tiles_n"], die_group=p["die_group"], grouped=1, split2=split2, cpd=n_cu // 8,
                           tiles_m_grp=p["tiles_m"] // ngrp)
            if p["order"]:
                for order, ndead in _orders(p["tiles_m"] * p["tiles_n"], True, rng):
                    _cover(tiles, args, p["nwg"], order, ndead)
            else:
                _cover(tiles, args, p["nwg"])
    assert {k[3] for k in seen} == {0, 1} and {k[5] for k in seen} == {0, 1}


@pytest.mark.parametrize("tm,tn", ((8, 8), (16, 9), (9, 16), (3, 8), (7, 5)))
def test_placement_is_what_the_dies_are_promised(tiles, tm, tn):
    """die groups: a die (launch position mod 8) owns whole tile rows (1) or tile columns (2); otherwise the tile column
    of the linear index is skewed by the tile row"""
    def coords(args, t):
        r, c = C.c_int(), C.c_int()
        tiles.emu_tile_coords(args, t, C.byref(r), C.byref(c))
        return r.value, c.value
    for die_group in (0, 1, 2):
        if (die_group == 1 and tm % 8) or (die_group == 2 and tn % 8):
            continue          # (the plans group by die only where the rows / columns divide among the eight dies)
        args = _launch(tm, tn, die_group=die_group)
        got = [coords(args, t) for t in range(tm * tn)]
        assert sorted(got) == [(r, c) for r in range(tm) for c in range(tn)]
        for t, (r, c) in enumerate(got):
            if die_group == 1:
                assert r % 8 == t % 8
            elif die_group == 2:
                assert c % 8 == t % 8
            else:
                assert (r, c) == (t // tn, (t % tn + t // tn) % tn)
    assert coords(_launch(tm, tn, skew=0), tn + 1) == (1, 1)


SPLIT2_GRIDS = ((1, 8), (8, 1), (2, 4), (2, 8), (4, 4), (16, 1), (3, 8), (24, 1), (1, 5), (5, 1), (3, 3), (9, 1), (1, 9))


@pytest.mark.parametrize("tm,tn", SPLIT2_GRIDS)
def test_halved_launches_map_positions_one_to_one(tiles, tm, tn):
    """split2 with 8, 16, 24 tiles (paired through cpd) and 5, 9 tiles (plain); cpd below, at and above 2 ntile / 8"""
    ntile, rng = tm * tn, random.Random(tm * 100 + tn)
    m2 = 2 * (ntile // 8)
    for cpd in sorted({1, max(m2 - 1, 1), max(m2, 1), m2 + 1, 32}):
        args = _launch(tm, tn, grouped=1, split2=1, cpd=cpd, tiles_m_grp=tm)
        _cover(tiles, args, 2 * ntile)
        for order, ndead in _orders(ntile, True, rng):
            _cover(tiles, args, 2 * ntile, order, ndead)
        pos = (C.c_int * (6 * ntile))()
        tiles.emu_launch_positions(args, 2 * ntile, pos)
        bs, t, half = (np.array(pos[i::3]) for i in range(3))
        assert (bs == half).all()
        if ntile % 8 == 0:
            # on a die (position mod 8) the first cpd positions get a compute unit each and the next cpd join them: the
            # unit with the q-th heaviest half of the order in the first round has the q-th lightest in the second
            assert (t % 8 == np.arange(2 * ntile) % 8).all()
            q = (t // 8) * 2 + half
            for die in range(8):
                qd = q[die::8]
                assert sorted(qd) == list(range(m2))
                for r in range(cpd, min(2 * cpd, m2)):
                    assert qd[r] + qd[r - cpd] == m2 - 1
        else:
            assert (t == np.arange(2 * ntile) // 2).all() and (half == np.arange(2 * ntile) % 2).all()


def _flag_cases():
    """(flag bytes of nkw words, nkt): 1, 2 and 3 words, ranges that end inside a word, density 0, one tile, ~half, all"""
    rng = np.random.default_rng(7)
    for nkw, nkt in ((1, 1), (1, 5), (1, 7), (1, 8), (2, 9), (2, 13), (2, 15), (2, 16), (3, 17), (3, 20), (3, 23), (3, 24)):
        for density in ("none", "one", "half", "all"):
            f = np.zeros(nkw * 8, dtype=np.uint8)
            if density == "one":
                f[rng.integers(nkt)] = 1
            elif density == "half":
                f[:nkt] = rng.integers(0, 2, nkt)
            elif density == "all":
                f[:nkt] = 1
            yield f, nkt


def _walk(tiles, a, b, lo, hi):
    out = (C.c_int * (len(a) + 1))()
    n = tiles.emu_flag_walk(a.ctypes.data, b.ctypes.data if b is not None else None, lo, hi, out)
    return list(out[:n])


def test_flag_walk_returns_the_flagged_tiles_of_the_range(tiles):
    rng = np.random.default_rng(11)
    for f, nkt in _flag_cases():
        other = np.ones_like(f)
        other[:nkt] = rng.integers(0, 2, nkt)
        for b in (None, other):
            both = f if b is None else f & b
            for lo, hi in {(0, nkt), (0, max(nkt - 3, 0)), (min(2, nkt), nkt), (nkt // 2, nkt), (nkt, nkt), (3, 3)}:
                lo, hi = min(lo, hi), hi
                for beyond in (0, 1):
                    # set bytes at and beyond the end of the range must be ignored
                    a = f.copy()
                    if beyond:
                        a[hi:] = 1
                    want = [k for k in range(lo, hi) if both[k]]
                    assert _walk(tiles, a, b, lo, hi) == want, (f.tolist(), nkt, lo, hi, beyond, b is not None)
                    if b is None:       # no flagged tile left in the range: the end of the range itself
                        for frm in range(lo, hi + 1):
                            nxt = [k for k in want if k >= frm]
                            assert tiles.emu_next_flagged(a.ctypes.data, frm, hi) == (nxt[0] if nxt else hi)


def test_split2_halves_are_disjoint_and_cover(tiles):
    for f, nkt in _flag_cases():
        nkw = len(f) // 8
        for beyond in (0, 1, 0xff):
            a = f.copy()
            a[nkt:] = beyond                 # (flag bytes beyond the last K tile are never written: anything)
            occupied = [k for k in range(nkt) if f[k]]
            n = len(occupied)
            got = []
            for half in (0, 1):
                lo, hi = C.c_int(-1), C.c_int(-1)
                tiles.emu_half_range(a.ctypes.data, nkw, nkt, half, C.byref(lo), C.byref(hi))
                assert 0 <= lo.value <= hi.value <= nkt, (f.tolist(), nkt, half, lo.value, hi.value)
                # (the K loop walks the stored flags of the range)
                got.append((lo.value, hi.value, _walk(tiles, f, None, lo.value, hi.value)))
            (lo0, hi0, k0), (lo1, hi1, k1) = got
            assert lo0 == 0 and hi0 == lo1 and hi1 == nkt                  # adjacent ranges: disjoint
            assert k0 + k1 == occupied                                      # every occupied tile, once
            assert len(k0) == n // 2 and len(k1) == n - n // 2, (f.tolist(), nkt, k0, k1)
