"""CPU check of the launch plans of the contraction kernel (renormalizer_amd/csrc/mpse_plans.h: launch_plan,
grouped_plan - what gemm_impl and gemm_grouped of mpse_gemm.hip read) against their restatement in Python
(tests/gemm_policy.py), which tests/test_gemm_gpu.py in turn holds against the path counters of real launches.
  * every row of the GPU test's table, for 256, 304, 64 and 8 compute units: the counters the C plan raises are those
    `expected_paths` names;
  * a grid of small shapes on both sides of every threshold of the policy: every field of both plans.
The plans are compiled with g++ from tests/host_emu; no GPU needed."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import gemm_policy as P   # (tests/gemm_policy.py)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUS = (256, 304, 64, 8)
PLAIN_FIELDS = ("tiles_m", "tiles_n", "nkt", "ksplit", "kt_per_split", "ws_bytes", "leave_slices", "nwg", "fast", "wide",
                "masks", "nkw", "order", "die_group", "rgx", "rgy", "dot_producers")
GROUPED_FIELDS = ("tiles_m", "tiles_n", "nkw", "die_group", "order", "wide", "nwg")
# (both K maps single level, strides and spans the fast kernel can address) of the operand layouts of the GPU table
LAYOUT_FLAGS = {"rowmajor": (1, 1), "gaps": (1, 1), "trans": (1, 1), "twolevel": (0, 1), "reversed": (1, 0), "span": (1, 0)}
DTYPES = ((0, 0), (1, 0), (0, 1), (1, 1))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_gemm_plan") / "libplan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "plan_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    for fn in (lib.emu_gemm_launch_plan, lib.emu_gemm_grouped_plan):
        fn.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        fn.restype = None
    return lib


def c_plain(lib, n_cu, M, N, K, batch, ca=0, cb=0, hint=0, k_single=1, fast_ok=1, dot_cap=None, slices_cap=None, beta=0):
    args = (C.c_longlong * 15)(M, N, K, batch, n_cu, ca, cb, hint, k_single, fast_ok, dot_cap is not None, dot_cap or 0,
                               slices_cap is not None, slices_cap or 0, beta)
    out = (C.c_longlong * len(PLAIN_FIELDS))()
    lib.emu_gemm_launch_plan(args, out)
    return dict(zip(PLAIN_FIELDS, out))


def c_grouped(lib, n_cu, M, N, ngrp, nkt_max, any_mask, split2, ca):
    args = (C.c_longlong * 8)(M, N, ngrp, nkt_max, any_mask, split2, ca, n_cu)
    out = (C.c_longlong * len(GROUPED_FIELDS))()
    lib.emu_gemm_grouped_plan(args, out)
    return dict(zip(GROUPED_FIELDS, out))


@pytest.mark.parametrize("n_cu", N_CUS)
def test_table_rows_reach_their_paths(emu, n_cu):
    for name, (dims, kind, _sparse, hints, *_rest) in P.CASES.items():
        M, N, K, batch = dims(n_cu)
        P._shape_preconditions(name, n_cu, M, N, K, batch)
        k_single, fast_ok = LAYOUT_FLAGS[kind]
        for (ca, cb), hint in itertools.product(DTYPES, hints):
            plan = c_plain(emu, n_cu, M, N, K, batch, ca, cb, hint, k_single, fast_ok, beta=1)
            want = P.expected_paths(name, n_cu, M, N, K, batch, hint)
            assert P.paths_of_plan(plan, batch) == want, (name, n_cu, ca, cb, hint, plan)


def _tile_grids(n_cu):
    """(tile rows, tile columns, batch) on both sides of every tile-count threshold of the policy"""
    counts = {1, 2, 63, 64, 65, 2 * n_cu, 2 * n_cu + 1, 2048, 2049}
    grids = set()
    for batch in (1, 3):
        for target in (n_cu - 1, n_cu, n_cu + 1):             # tiles * batch around the fill target
            counts_b = {max(1, target // batch), target // batch + 1}
            for t in counts_b | (counts if batch == 1 else {64, 65}):
                # as one row, one column, and every split with a side of 7, 8 or 16 (multiples of 8 and not)
                grids |= {(t, 1, batch), (1, t, batch)}
                grids |= {(s, t // s, batch) for s in (7, 8, 16) if t % s == 0} | {(t // s, s, batch) for s in (7, 8, 16) if t % s == 0}
    return sorted(grids)


def _check(got, want, what):
    assert got == want, (what, {k: (got[k], want[k]) for k in want if got[k] != want[k]})


@pytest.mark.parametrize("n_cu", N_CUS)
def test_plain_plan_on_the_boundary_grid(emu, n_cu):
    flags = list(itertools.product((0, 1, 2, 3), ((1, 1), (1, 0), (0, 1), (0, 0))))
    n = 0
    for (tm, tn, batch), nkt, ragged in itertools.product(_tile_grids(n_cu), (1, 2, 3, 4, 5, 8, 9), (0, 1)):
        M, N, K = 64 * tm - 13 * ragged, 64 * tn - 7 * ragged, 16 * nkt - 5 * ragged
        for i, (hint, (k_single, fast_ok)) in enumerate(flags):
            ca, cb = DTYPES[(i + tm + nkt) % 4]
            kw = dict(ca=ca, cb=cb, hint=hint, k_single=k_single, fast_ok=fast_ok, beta=i & 1)
            _check(c_plain(emu, n_cu, M, N, K, batch, **kw), P.plain_plan(n_cu, M, N, K, batch, **kw), (M, N, K, batch, kw))
            n += 1
        for ca, cb in DTYPES:
            # dot request: room below, at and above the number of producers, and for less than one row of the reduction
            full = P.plain_plan(n_cu, M, N, K, batch, ca, cb, dot_cap=1 << 40)
            producers = full["dot_producers"] or full["nwg"]
            for cap in {1, full["rgx"] - 1, producers - 1, producers, producers + 1} - {0, -1}:
                kw = dict(ca=ca, cb=cb, dot_cap=cap)
                _check(c_plain(emu, n_cu, M, N, K, batch, **kw), P.plain_plan(n_cu, M, N, K, batch, **kw), (M, N, K, batch, kw))
            # slice offer: room below and at the workspace bytes, with and without a beta term or a dot request
            ws = full["ws_bytes"]
            for cap, beta, dot in itertools.product((ws - 1, ws), (0, 1), (None, 1 << 40)):
                kw = dict(ca=ca, cb=cb, slices_cap=max(cap, 0), beta=beta, dot_cap=dot)
                _check(c_plain(emu, n_cu, M, N, K, batch, **kw), P.plain_plan(n_cu, M, N, K, batch, **kw), (M, N, K, batch, kw))
                n += 1
    assert n > 1000


def test_masks_stop_at_16384_batch_elements(emu):
    for batch, hint in itertools.product((16383, 16384, 16385), (0, 1, 2, 3)):
        got, want = c_plain(emu, 256, 70, 50, 100, batch, hint=hint), P.plain_plan(256, 70, 50, 100, batch, hint=hint)
        _check(got, want, (batch, hint))
        assert got["masks"] == int(hint != 0 and batch <= 16384)


@pytest.mark.parametrize("n_cu", N_CUS)
def test_grouped_plan_on_the_boundary_grid(emu, n_cu):
    for (tm, tn, _b), ngrp in itertools.product(_tile_grids(n_cu), (1, 2, 8)):
        if tm % ngrp:
            continue
        M, N = 64 * (tm // ngrp) - (13 if ngrp == 1 else 0), 64 * tn - 7     # (several groups: whole tile rows)
        # K tiles of the longest group around the 64 flag words of a tile's LDS copy
        for nkt_max, any_mask, split2, ca in itertools.product((1, 8, 9, 512, 513), (0, 1), (0, 1), (0, 1)):
            args = (n_cu, M, N, ngrp, nkt_max, any_mask, split2 and ngrp == 1, ca)
            _check(c_grouped(emu, *args), P.grouped_plan(*args), args)


def test_grid_straddles_every_threshold(emu):
    """the grid above reaches both sides of each decision (256 compute units)"""
    seen = {f: set() for f in PLAIN_FIELDS}
    for (tm, tn, batch), nkt, hint in itertools.product(_tile_grids(256), (1, 2, 3, 4, 5, 8, 9), (0, 3)):
        for cap in (None, 4):
            p = c_plain(emu, 256, 64 * tm, 64 * tn, 16 * nkt, batch, 1, 1, hint, dot_cap=cap, slices_cap=1 << 20)
            for f in PLAIN_FIELDS:
                seen[f].add(p[f])
    for f in ("leave_slices", "wide", "masks", "order"):
        assert seen[f] == {0, 1}, f
    assert seen["die_group"] == {0, 1, 2} and len(seen["ksplit"]) > 2 and {0, 4} <= seen["dot_producers"]
