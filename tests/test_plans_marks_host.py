"""CPU check of the marks that the planners set on their steps (renormalizer_amd/csrc/mpse_plans.h: `marked`) and of the
hand-off of K slices they describe.  The expected marks come from a model of the step lists written here, with the
rules of the marks applied to it in Python; the emulator (tests/host_emu/plan_emu.cpp) only reports what the header set.
The hand-off itself is forced in the emulator (emu_set_slice_handoff): the product stores K slices instead of its range of
T1, which stays poisoned, and the elementwise MPO step sums them by the address formula of the device kernel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from renormalizer_amd import engine as E
from contract_refs import rand, ref_env, ref_heff             # (tests/contract_refs.py)
from test_plans_host import emu_env, emu_heff                 # (the ctypes callers of tests/test_plans_host.py)
from test_plans_epi_host import _heff, _operands, _site       # (sites and hooks of the folded plan)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_GEMM, K_COPY, K_WMIX, K_GGEMM = 0, 1, 2, 3


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_marks") / "libplan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "plan_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_heff_apply.argtypes = [C.c_int, C.POINTER(E.mpse_heff), C.c_void_p, C.c_void_p]
    lib.emu_env_update.argtypes = [C.c_int, C.c_int, C.POINTER(E.mpse_dims), C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.emu_heff_marks.argtypes = [C.c_int, C.POINTER(E.mpse_heff), C.c_int, C.POINTER(C.c_longlong), C.c_longlong]
    lib.emu_heff_marks.restype = C.c_longlong
    lib.emu_env_marks.argtypes = [C.c_int, C.c_int, C.POINTER(E.mpse_dims), C.c_int, C.c_int, C.POINTER(C.c_longlong),
                                  C.c_longlong]
    lib.emu_env_marks.restype = C.c_longlong
    lib.emu_set_unit_threshold.argtypes = [C.c_longlong]
    lib.emu_set_fold_min.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong]
    lib.emu_set_slice_handoff.argtypes = [C.c_int]
    lib.emu_set_unit_threshold(0)        # a unit channel splits the products at every size
    return lib


# ------------------------------------------------------------------------------------ a model of the step lists
def _step(kind=K_GEMM, c="OUT", c_off=0, m=0, n=0, batch=1, beta=0, cin=False, w=None, w_real=True, reads=None, ngrp=0):
    """what the rules of the marks look at; w = (Da, wl, d, wr, N) for an MPO step written by push_w"""
    return dict(kind=kind, c=c, c_off=c_off, m=m, n=n, batch=batch, beta=beta, cin=cin, w=w, w_real=w_real, reads=reads,
                ngrp=ngrp)


def _env_times(rows, w, N, unit, square, outer=True):
    """X = E . K into T1: a copy for the unit channel (1-based; 0 = none) and a product for each run of the others"""
    u = unit - 1 if 1 <= unit <= w and square else -1
    steps = [_step(K_COPY, c="T1")] if u >= 0 else []
    for b0, nb in ((0, u if u >= 0 else w), (u + 1, w - u - 1 if u >= 0 else 0)):
        if nb > 0:
            steps.append(_step(c="T1", c_off=b0 * rows * N if outer else b0 * N, m=nb * rows, n=N))
    return steps


def model_heff(Dl, d, Dr, wl, wr, nsite=1, l_unit=0, d1=1, wm=1):
    """plan_heff without a unit channel on the right; bra bonds = ket bonds, no ancilla"""
    if nsite == 0:
        return _env_times(Dl, wl, Dr, l_unit, True, outer=False) + [_step()]
    if nsite == 1:
        N = d * Dr
        return _env_times(Dl, wl, N, l_unit, True) + [_step(c="T2", batch=Dl, w=(Dl, wl, d, wr, Dr), reads="T1"), _step()]
    n1 = d1 * Dr
    return (_env_times(Dl, wl, d * n1, l_unit, True) + [_step(c="T2", batch=Dl, w=(Dl, wl, d, wm, n1), reads="T1"),
                                                        _step(c="T3", batch=Dl * d, reads="T2"), _step()])


def model_env(dom, Dl, d, Dr, wl, wr, env_unit=0):
    if dom == "L":
        N = d * Dr
        return _env_times(Dl, wl, N, env_unit, True) + [_step(c="T2", batch=Dl, w=(Dl, wl, d, wr, Dr), reads="T1"), _step()]
    return [_step(c="T1", m=Dl * d, n=wr * Dr), _step(c="T2", batch=Dl, reads="T1"), _step()]      # no push_w step


def expected_marks(steps):
    """the rules of the marks, applied to the model: (kind, elementwise_w, slices_to, b_lo, b_hi, slice_elems, completes)"""
    ew = []
    for s in steps:
        w = s["w"]
        ew.append(bool(s["kind"] == K_GEMM and w and s["w_real"] and s["c_off"] == 0 and s["beta"] == 0
                       and w[1] * w[2] <= 16 and w[2] * w[3] <= 16))
    cons = next((i for i, s in enumerate(steps) if ew[i] and s["reads"] == "T1"), None)
    marks = [[s["kind"], int(ew[i]), -1, 0, 0, 0, 0] for i, s in enumerate(steps)]
    if cons is not None:
        prods = [i for i in range(cons) if steps[i]["kind"] == K_GEMM and not steps[i]["w"] and steps[i]["c"] == "T1"]
        Da, _, dd, _, N = steps[cons]["w"]
        if len(prods) == 1:
            p = steps[prods[0]]
            if (p["batch"] == 1 and p["beta"] == 0 and not p["cin"] and p["n"] == dd * N and p["m"] % Da == 0
                    and p["c_off"] % (Da * dd * N) == 0):
                marks[prods[0]][2] = cons
                lo = p["c_off"] // (Da * dd * N)
                marks[cons][3:6] = [lo, lo + p["m"] // Da, p["m"] * p["n"]]
    last = steps[-1]
    if last["kind"] == K_GEMM:
        marks[-1][6] = int(last["c"] == "OUT" and last["c_off"] == 0 and last["batch"] == 1)
    elif last["kind"] == K_GGEMM:
        marks[-1][6] = int(last["ngrp"] == 1 and last["c"] == "OUT" and last["c_off"] == 0)
    return [tuple(m) for m in marks]


# ------------------------------------------------------------------------------------ the header's marks
def _heff_struct(Dl, d, Dr, wl, wr, nsite, l_unit, d1, wm):
    h = E.mpse_heff()
    h.nsite, h.l_unit, h.r_unit = nsite, l_unit, 0
    dm = h.dims
    dm.Dl_ket = dm.Dl_bra = Dl
    dm.Dr_ket = dm.Dr_bra = Dr
    dm.danc, dm.wl, dm.wr, dm.d0, dm.d1, dm.wm = 1, wl, wr, d, d1, wm
    return h


def _records(n, rec):
    assert n > 0 and n % 7 == 0
    return [tuple(rec[i:i + 7]) for i in range(0, n, 7)]


def heff_marks(emu, cplx, Dl, d, Dr, wl, wr, nsite=1, l_unit=0, d1=1, wm=1):
    h = _heff_struct(Dl, d, Dr, wl, wr, nsite, l_unit, d1, wm)
    h.l_dtype = h.r_dtype = E.C128 if cplx else E.F64
    h.w_dtype = E.F64
    rec = (C.c_longlong * 256)()
    return _records(emu.emu_heff_marks(E.C128 if cplx else E.F64, C.byref(h), 0, rec, 256), rec)


def env_marks(emu, cplx, dom, Dl, d, Dr, wl, wr, env_unit=0):
    dm = E.mpse_dims()
    dm.Dl_ket = dm.Dl_bra = Dl
    dm.Dr_ket = dm.Dr_bra = Dr
    dm.danc, dm.wl, dm.wr, dm.d0, dm.env_unit = 1, wl, wr, d, env_unit
    dt = E.C128 if cplx else E.F64
    rec = (C.c_longlong * 256)()
    return _records(emu.emu_env_marks(dt, 0 if dom == "L" else 1, C.byref(dm), dt, E.F64, rec, 256), rec)


@pytest.mark.parametrize("cplx", [False, True])
def test_marks_one_site(emu, cplx):
    Dl, d, Dr, wl, wr = 6, 2, 5, 3, 3
    got = heff_marks(emu, cplx, Dl, d, Dr, wl, wr)
    assert got == expected_marks(model_heff(Dl, d, Dr, wl, wr))
    # [product -> T1, W step, product -> out]: the hand-off over all three channels, the last step completes
    assert got == [(K_GEMM, 0, 1, 0, 0, 0, 0), (K_GEMM, 1, -1, 0, 3, wl * Dl * d * Dr, 0), (K_GEMM, 0, -1, 0, 0, 0, 1)]
    # a unit channel in the middle: two products write T1, nobody hands over; the W step stays elementwise
    got = heff_marks(emu, cplx, Dl, d, Dr, wl, wr, l_unit=2)
    assert got == expected_marks(model_heff(Dl, d, Dr, wl, wr, l_unit=2))
    assert [g[0] for g in got] == [K_COPY, K_GEMM, K_GEMM, K_GEMM, K_GEMM]
    assert all(g[2] == -1 for g in got) and [g[1] for g in got] == [0, 0, 0, 1, 0] and got[-1][6] == 1
    # a unit channel at the edge: one product over the channels [1, 3), into T1 behind the copied channel
    got = heff_marks(emu, cplx, Dl, d, Dr, wl, wr, l_unit=1)
    assert got == expected_marks(model_heff(Dl, d, Dr, wl, wr, l_unit=1))
    assert got[1][2] == 2 and got[2][1:6] == (1, -1, 1, 3, 2 * Dl * d * Dr)
    # wl * d = 20 > 16: the MPO step runs as a product, no hand-off
    got = heff_marks(emu, cplx, 6, 4, 5, 5, 3)
    assert got == expected_marks(model_heff(6, 4, 5, 5, 3))
    assert all(g[1] == 0 and g[2] == -1 for g in got) and len(got) == 3 and got[-1][6] == 1


@pytest.mark.parametrize("cplx", [False, True])
def test_marks_two_site_zero_site_and_env(emu, cplx):
    Dl, d, Dr, wl, wr, wm, d1 = 5, 2, 4, 3, 3, 3, 2
    got = heff_marks(emu, cplx, Dl, d, Dr, wl, wr, nsite=2, d1=d1, wm=wm)
    assert got == expected_marks(model_heff(Dl, d, Dr, wl, wr, nsite=2, d1=d1, wm=wm))
    # only the first MPO step is the consumer; the step of the second site is an ordinary batched product
    assert [g[1] for g in got] == [0, 1, 0, 0] and got[0][2] == 1 and got[1][3:6] == (0, 3, wl * Dl * d * d1 * Dr)
    assert got[-1][6] == 1
    got = heff_marks(emu, cplx, 6, 1, 5, 3, 3, nsite=0)
    assert got == expected_marks(model_heff(6, 1, 5, 3, 3, nsite=0))
    assert got == [(K_GEMM, 0, -1, 0, 0, 0, 0), (K_GEMM, 0, -1, 0, 0, 0, 1)]
    got = env_marks(emu, cplx, "L", 6, 2, 5, 3, 3)
    assert got == expected_marks(model_env("L", 6, 2, 5, 3, 3))
    assert got[0][2] == 1 and got[1][1:6] == (1, -1, 0, 3, 3 * 6 * 2 * 5) and got[2][6] == 1
    got = env_marks(emu, cplx, "R", 6, 2, 5, 3, 3)
    assert got == expected_marks(model_env("R", 6, 2, 5, 3, 3))
    assert all(g[1] == 0 and g[2] == -1 for g in got) and got[-1][6] == 1


def test_marks_folded_plan(emu):
    """the folded plan has no small-site MPO step; its last grouped step, one group into `out`, completes - the last
    of two where the products with R take two launches"""
    emu.emu_set_fold_min(1, 4, 1)
    try:
        rng = np.random.default_rng(7)
        for kind, D, d, wr, fold, kinds in (("penta", 16, 4, 4, 1, [K_GGEMM, K_WMIX, K_GGEMM]),
                                            ("penta", 16, 4, 4, 2, [K_GGEMM, K_GGEMM]),
                                            ("many", 8, 4, 7, 2, [K_GGEMM, K_GGEMM, K_GGEMM])):
            w0 = _site(rng, d, kind, wr)
            l, r, c = _operands(rng, D, d, w0, True)
            h, keep = _heff(l, r, w0, c, 1, wr)
            rec = (C.c_longlong * 256)()
            got = _records(emu.emu_heff_marks(E.C128, C.byref(h), fold, rec, 256), rec)
            model = [_step(k, c="T", ngrp=2) for k in kinds[:-1]]
            if kind == "many":
                model[-1] = _step(K_GGEMM, ngrp=1)                 # the first launch of the products with R
            model.append(_step(K_GGEMM, ngrp=1))
            assert got == expected_marks(model), (kind, fold)
            assert [g[0] for g in got] == kinds and [g[6] for g in got] == [0] * (len(kinds) - 1) + [1]
            assert all(g[1] == 0 and g[2] == -1 for g in got)
    finally:
        emu.emu_set_fold_min(1 << 28, 64, 8)


# ------------------------------------------------------------------------------------ the hand-off, emulated
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("case", ["one_site", "one_site_unit_edge", "two_site", "env_L"])
def test_emulated_slice_handoff(emu, case, cplx):
    rng = np.random.default_rng(31)
    if case == "two_site":
        Dl, d, Dr, wl, wr, wm, d1 = 5, 2, 4, 3, 3, 3, 2
        ws = [rand(rng, (wl, d, d, wm), False), rand(rng, (wm, d1, d1, wr), False)]
        c = rand(rng, (Dl, d, d1, Dr), cplx)
    else:
        Dl, d, Dr, wl, wr = 6, 2, 5, 3, 3
        ws = [rand(rng, (wl, d, d, wr), False)]
        c = rand(rng, (Dl, d, Dr), cplx)
    l, r = rand(rng, (Dl, wl, Dl), cplx), rand(rng, (Dr, wr, Dr), cplx)
    unit = 0
    if case == "one_site_unit_edge":
        unit = 1
        l[:, 0, :] = np.eye(Dl)
    if case == "env_L":
        ref = ref_env("L", l, c, ws[0])
        run = lambda: emu_env(emu, l, c, ws[0], "L")
    else:
        ref = ref_heff(l, r, ws, c)
        run = lambda: emu_heff(emu, l, r, ws, c, l_unit=unit)
    tol = 1e-11 * np.abs(ref).max()
    plain = run()
    assert np.abs(plain - ref).max() < tol
    try:
        for S in (2, 3):
            emu.emu_set_slice_handoff(S)
            got = run()
            assert got.shape == ref.shape
            assert np.abs(got - plain).max() < tol, S
            assert np.abs(got - ref).max() < tol, S
    finally:
        emu.emu_set_slice_handoff(0)
