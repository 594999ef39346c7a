"""The NumPy references of tests/contract_refs.py (written from include/mpsengine.h) against the host emulation of the
contraction plans (tests/host_emu), at small shapes whose extents all differ: the references of the device tests
tests/test_unit_channel_gpu.py and tests/test_ft_contract_gpu.py agree with what the plans compute before either is
held against the device, so a disagreement there points at device code.  The unit threshold of the emulation is zero:
the plans take the copy / beta-source shortcuts at these sizes.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from renormalizer_amd import engine as E

import contract_refs as cr
from contract_refs import UP, DOWN, rand
from test_plans_host import emu_heff, emu_env          # the argument marshalling of the one-layer emulation
from test_plans_ft_host import _term                    # ... and of the two-layer one

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-13      # small shapes, sums of at most a few hundred terms of O(1): rounding stays far below


def _build(tmp, name):
    out = str(tmp / ("lib" + name + ".so"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", name + ".cpp"), "-o", out])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def emu1(tmp_path_factory):
    lib = _build(tmp_path_factory.mktemp("refs_emu"), "plan_emu")
    lib.emu_heff_apply.argtypes = [C.c_int, C.POINTER(E.mpse_heff), C.c_void_p, C.c_void_p]
    lib.emu_env_update.argtypes = [C.c_int, C.c_int, C.POINTER(E.mpse_dims), C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.emu_set_unit_threshold.argtypes = [C.c_longlong]
    lib.emu_set_unit_threshold(0)
    return lib


@pytest.fixture(scope="module")
def emu2(tmp_path_factory):
    lib = _build(tmp_path_factory.mktemp("refs_emu_ft"), "plan_emu_ft")
    lib.emu_heff_apply_ft.argtypes = [C.c_int, C.POINTER(E.mpse_heff_ft), C.c_void_p, C.c_void_p]
    lib.emu_env_update_ft.argtypes = [C.c_int, C.c_int, C.POINTER(E.mpse_heff_ft), C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p]
    return lib


def _unit_env(rng, D, w, u, cplx):
    e = rand(rng, (D, w, D), cplx)
    if u is not None:
        e[:, u, :] = np.eye(D)
    return e


@pytest.mark.parametrize("cplx,cplx_env", [(False, False), (True, False), (True, True)])
def test_heff_reference_vs_emulated_plans(emu1, cplx, cplx_env):
    """0-, 1- and 2-site centres, with and without ancilla legs, unit channel first / inside / last on either side"""
    rng = np.random.default_rng(3)
    Dl, Dr, d0, d1, a0, a1, wl, wm, wr = 5, 7, 3, 2, 2, 3, 4, 3, 5
    for ul, ur in ((0, 0), (1, 2), (3, 4), (2, 0)):
        l, r = _unit_env(rng, Dl, wl, ul, cplx_env), _unit_env(rng, Dr, wr, ur, cplx_env)
        w0, w0m, w1 = rand(rng, (wl, d0, d0, wr), False), rand(rng, (wl, d0, d0, wm), False), rand(rng, (wm, d1, d1, wr), False)
        for lu, ru in ((ul + 1, ur + 1), (ul + 1, 0), (0, ur + 1), (0, 0)):
            for shape, ws in (((Dl, d0, Dr), [w0]), ((Dl, d0, a0, Dr), [w0]), ((Dl, d0, d1, Dr), [w0m, w1]),
                              ((Dl, d0, a0, d1, a1, Dr), [w0m, w1])):
                c = rand(rng, shape, cplx)
                ref = cr.ref_heff(l, r, ws, c)
                got = emu_heff(emu1, l, r, ws, c, l_unit=lu, r_unit=ru)
                assert got.shape == ref.shape and cr.relerr(got, ref) < BOUND, (shape, lu, ru)
            r0 = _unit_env(rng, Dr, wl, ul, cplx_env)
            c = rand(rng, (Dl, Dr), cplx)
            ref = cr.ref_heff(l, r0, [], c)
            got = emu_heff(emu1, l, r0, [], c, l_unit=lu, r_unit=lu)
            assert cr.relerr(got, ref) < BOUND, ("0-site", lu)
    # bra bonds != ket bonds
    l, r = rand(rng, (4, wl, Dl), cplx_env), rand(rng, (6, wr, Dr), cplx_env)
    c = rand(rng, (Dl, d0, a0, Dr), cplx)
    ref = cr.ref_heff(l, r, [w0], c)
    got = emu_heff(emu1, l, r, [w0], c, l_unit=1, r_unit=1)
    assert got.shape == ref.shape == (4, d0, a0, 6) and cr.relerr(got, ref) < BOUND


@pytest.mark.parametrize("cplx", [False, True])
def test_env_reference_vs_emulated_plans(emu1, cplx):
    rng = np.random.default_rng(4)
    Dl, Dr, d, da, wl, wr = 5, 7, 3, 2, 4, 6
    w = rand(rng, (wl, d, d, wr), False)
    for anc in (False, True):
        shape = (Dl, d, da, Dr) if anc else (Dl, d, Dr)
        ket, bra = rand(rng, shape, cplx), rand(rng, shape, cplx)
        for dom, D, we in (("L", Dl, wl), ("R", Dr, wr)):
            for u in (0, 2, we - 1):
                env = _unit_env(rng, D, we, u, cplx)
                for unit in (0, u + 1):
                    ref = cr.ref_env(dom, env, ket, w)
                    assert cr.relerr(emu_env(emu1, env, ket, w, dom, env_unit=unit), ref) < BOUND, (dom, anc, u)
                    ref = cr.ref_env(dom, env, ket, w, bra=bra)
                    assert cr.relerr(emu_env(emu1, env, ket, w, dom, bra=bra, env_unit=unit), ref) < BOUND
                    ref = cr.ref_env(dom, env, ket, w, bra=bra, bra_conj=False)
                    assert cr.relerr(emu_env(emu1, env, ket, w, dom, bra=bra, bra_conj=False, env_unit=unit), ref) < BOUND
        # a bra with other bonds
        bshape = (4, d, da, 6) if anc else (4, d, 6)
        bra = rand(rng, bshape, cplx)
        for dom, env in (("L", rand(rng, (4, wl, Dl), cplx)), ("R", rand(rng, (6, wr, Dr), cplx))):
            ref = cr.ref_env(dom, env, ket, w, bra=bra)
            got = emu_env(emu1, env, ket, w, dom, bra=bra, env_unit=1)
            assert got.shape == ref.shape and cr.relerr(got, ref) < BOUND, (dom, anc)


@pytest.mark.parametrize("cplx_env", [False, True])
@pytest.mark.parametrize("trans", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("legs", [(UP, UP), (UP, DOWN), (DOWN, DOWN)])
def test_two_layer_references_vs_emulated_plans(emu2, legs, trans, cplx_env):
    rng = np.random.default_rng(5)
    Dl, du, dv, Dr = 5, 3, 4, 7
    wl1, wr1, wl2, wr2 = 2, 3, 4, 5
    d1 = du if legs[0] == UP else dv
    d2 = du if legs[1] == UP else dv
    w1, w2 = rand(rng, (wl1, d1, d1, wr1), False), rand(rng, (wl2, d2, d2, wr2), False)
    l, r = rand(rng, (Dl, wl1, wl2, Dl), cplx_env), rand(rng, (Dr, wr1, wr2, Dr), cplx_env)
    for cplx in ((True,) if cplx_env else (False, True)):
        c = rand(rng, (Dl, du, dv, Dr), cplx)
        code = E.C128 if cplx else E.F64
        h = _term(l, r, w1, w2, legs, trans, c.shape)
        out = np.full(c.shape, np.nan, dtype=c.dtype)
        assert emu2.emu_heff_apply_ft(code, C.byref(h), c.ctypes.data, out.ctypes.data) == 0
        ref = cr.ref_apply_ft(l, r, w1, w2, legs, trans, c)
        assert ref.shape == out.shape and cr.relerr(out, ref) < BOUND
        for dom, env in (("L", l), ("R", r)):
            ref = cr.ref_env_ft(dom, env, w1, w2, legs, trans, c)
            out = np.full(ref.shape, np.nan, dtype=c.dtype)
            assert emu2.emu_env_update_ft(code, 0 if dom == "L" else 1, C.byref(h), env.ctypes.data,
                                          E.dtype_code(env.dtype), c.ctypes.data, out.ctypes.data) == 0
            assert out.shape == ((Dr, wr1, wr2, Dr) if dom == "L" else (Dl, wl1, wl2, Dl))
            assert cr.relerr(out, ref) < BOUND, dom
        # the dense matrix (the batch axes of the reference) is the reference applied to a vector
        if cplx:
            dense = cr.dense_ft(l, r, w1, w2, legs, trans, c.shape, chunk=100)
            ref = cr.ref_apply_ft(l, r, w1, w2, legs, trans, c)
            assert cr.relerr(dense @ c.ravel(), ref.ravel()) < BOUND
