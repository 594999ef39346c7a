"""CPU check of the plans behind mpse_heff_apply_ft / mpse_env_update_ft (renormalizer_amd/csrc/mpse_plans.h): two MPO
layers on a centre with two physical legs, each layer on the leg it names - the three terms of the finite-temperature
correction-vector operator and their environments.  The plans run on host memory through the naive executor of
tests/host_emu and are compared with numpy.einsum of the defining expressions on random operands whose extents all
differ, so that a swapped or transposed index changes the result.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from renormalizer_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP, DOWN = E.LEG_UP, E.LEG_DOWN
# (leg of layer 1, leg of layer 2): M1, M2, M3 of the operator a a X + 2 a X H + X H H
TERMS = {"M1": (UP, UP), "M2": (UP, DOWN), "M3": (DOWN, DOWN)}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_ft") / "libplan_emu_ft.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "plan_emu_ft.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_heff_apply_ft.argtypes = [C.c_int, C.POINTER(E.mpse_heff_ft), C.c_void_p, C.c_void_p]
    lib.emu_env_update_ft.argtypes = [C.c_int, C.c_int, C.POINTER(E.mpse_heff_ft), C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p]
    lib.emu_ft_steps_equal_heff2.argtypes = [C.c_int, C.POINTER(E.mpse_heff_ft)]
    return lib


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def _layer(w, trans):
    """MPO site as (left bond, leg out, leg in, right bond)"""
    return w.transpose(0, 2, 1, 3) if trans else w


def ref_apply(l, r, w1, w2, legs, trans, c):
    """out[d, u', v', k] of the term; l (a, b, c, d), r (j, g, i, k), c (a, u, v, j)"""
    a1, a2 = _layer(w1, trans[0]), _layer(w2, trans[1])
    if legs == (UP, UP):
        return np.einsum("abcd,bxug,cyxi,jgik,auvj->dyvk", l, a1, a2, r, c)
    if legs == (DOWN, DOWN):
        return np.einsum("abcd,bsvg,ctsi,jgik,auvj->dutk", l, a1, a2, r, c)
    return np.einsum("abcd,bxug,csvi,jgik,auvj->dxsk", l, a1, a2, r, c)


def ref_env(dom, env, w1, w2, legs, trans, x):
    a1, a2 = _layer(w1, trans[0]), _layer(w2, trans[1])
    xc = x.conj()
    if dom == "L":      # env (a, b, c, d) -> (j, g, i, k)
        expr = {(UP, UP): "abcd,bxug,cyxi,auvj,dyvk->jgik", (DOWN, DOWN): "abcd,bsvg,ctsi,auvj,dutk->jgik",
                (UP, DOWN): "abcd,bxug,csvi,auvj,dxsk->jgik"}[legs]
    else:               # env (j, g, i, k) -> (a, b, c, d)
        expr = {(UP, UP): "jgik,bxug,cyxi,auvj,dyvk->abcd", (DOWN, DOWN): "jgik,bsvg,ctsi,auvj,dutk->abcd",
                (UP, DOWN): "jgik,bxug,csvi,auvj,dxsk->abcd"}[legs]
    return np.einsum(expr, env, a1, a2, x, xc)


def _term(l, r, w1, w2, legs, trans, shape):
    h = E.mpse_heff_ft()
    h.Dl, h.d_up, h.d_down, h.Dr = shape
    h.wl1, h.wr1, h.wl2, h.wr2 = w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[3]
    h.leg1, h.leg2 = legs
    h.trans1, h.trans2 = trans
    h.W1, h.W2, h.w_dtype = w1.ctypes.data, w2.ctypes.data, E.dtype_code(w1.dtype)
    if l is not None:
        h.L, h.l_dtype = l.ctypes.data, E.dtype_code(l.dtype)
    if r is not None:
        h.R, h.r_dtype = r.ctypes.data, E.dtype_code(r.dtype)
    return h


def _operands(rng, legs, cplx, cplx_env=None):
    Dl, du, dv, Dr = 5, 3, 4, 7
    wl1, wr1, wl2, wr2 = 2, 3, 4, 5
    d1 = du if legs[0] == UP else dv
    d2 = du if legs[1] == UP else dv
    cplx_env = cplx if cplx_env is None else cplx_env
    l = _rand(rng, (Dl, wl1, wl2, Dl), cplx_env)
    r = _rand(rng, (Dr, wr1, wr2, Dr), cplx_env)
    w1 = _rand(rng, (wl1, d1, d1, wr1), False)
    w2 = _rand(rng, (wl2, d2, d2, wr2), False)
    c = _rand(rng, (Dl, du, dv, Dr), cplx)
    return l, r, w1, w2, c


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("trans", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("name", list(TERMS))
def test_term_apply(emu, name, trans, cplx):
    legs = TERMS[name]
    rng = np.random.default_rng(11)
    l, r, w1, w2, c = _operands(rng, legs, cplx)
    h = _term(l, r, w1, w2, legs, trans, c.shape)
    out = np.full(c.shape, np.nan, dtype=c.dtype)
    assert emu.emu_heff_apply_ft(E.C128 if cplx else E.F64, C.byref(h), c.ctypes.data, out.ctypes.data) == 0
    ref = ref_apply(l, r, w1, w2, legs, trans, c)
    assert np.abs(out - ref).max() < 1e-11 * np.abs(ref).max()


def test_real_environments_complex_centre(emu):
    rng = np.random.default_rng(12)
    for name, legs in TERMS.items():
        l, r, w1, w2, c = _operands(rng, legs, True, cplx_env=False)
        h = _term(l, r, w1, w2, legs, (0, 1), c.shape)
        out = np.full(c.shape, np.nan, dtype=c.dtype)
        assert emu.emu_heff_apply_ft(E.C128, C.byref(h), c.ctypes.data, out.ctypes.data) == 0
        ref = ref_apply(l, r, w1, w2, legs, (0, 1), c)
        assert np.abs(out - ref).max() < 1e-11 * np.abs(ref).max(), name


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("dom", ["L", "R"])
@pytest.mark.parametrize("trans", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("name", list(TERMS))
def test_term_environment(emu, name, trans, dom, cplx):
    legs = TERMS[name]
    rng = np.random.default_rng(13)
    l, r, w1, w2, x = _operands(rng, legs, cplx)
    env = l if dom == "L" else r
    h = _term(None, None, w1, w2, legs, trans, x.shape)
    ref = ref_env(dom, env, w1, w2, legs, trans, x)
    out = np.full(ref.shape, np.nan, dtype=x.dtype)
    st = emu.emu_env_update_ft(E.C128 if cplx else E.F64, 0 if dom == "L" else 1, C.byref(h), env.ctypes.data,
                               E.dtype_code(env.dtype), x.ctypes.data, out.ctypes.data)
    assert st == 0
    assert out.shape == ((7, 3, 5, 7) if dom == "L" else (5, 2, 4, 5))
    assert np.abs(out - ref).max() < 1e-11 * np.abs(ref).max()


def test_environment_then_apply_is_the_functional(emu):
    """<X| term |X> over two sites: the left environment of site 1 closes with the term applied to site 2."""
    rng = np.random.default_rng(14)
    for name, legs in TERMS.items():
        du, dv = 3, 4
        d1 = du if legs[0] == UP else dv
        d2 = du if legs[1] == UP else dv
        x1, x2 = _rand(rng, (1, du, dv, 6), True), _rand(rng, (6, du, dv, 1), True)
        wa1, wa2 = _rand(rng, (1, d1, d1, 3), False), _rand(rng, (1, d2, d2, 2), False)
        wb1, wb2 = _rand(rng, (3, d1, d1, 1), False), _rand(rng, (2, d2, d2, 1), False)
        one = np.ones((1, 1, 1, 1))
        h1 = _term(None, None, wa1, wa2, legs, (0, 1), x1.shape)
        env = np.full((6, 3, 2, 6), np.nan, dtype=complex)
        assert emu.emu_env_update_ft(E.C128, 0, C.byref(h1), one.ctypes.data, E.F64, x1.ctypes.data, env.ctypes.data) == 0
        h2 = _term(env, one, wb1, wb2, legs, (0, 1), x2.shape)
        out = np.full(x2.shape, np.nan, dtype=complex)
        assert emu.emu_heff_apply_ft(E.C128, C.byref(h2), x2.ctypes.data, out.ctypes.data) == 0
        val = np.vdot(x2, out)
        # dense: the operator on the two-site vector X[u1, v1, u2, v2]
        X = np.einsum("auvj,jxyk->uvxy", x1, x2)
        a1, b1 = wa1, wb1.transpose(0, 1, 2, 3)
        a2, b2 = _layer(wa2, 1), _layer(wb2, 1)
        if legs == (UP, UP):
            Y = np.einsum("opug,gqxh,ocpi,ieqh,uvxy->cvey", a1, b1, _layer(wa2, 1), _layer(wb2, 1), X)
        elif legs == (DOWN, DOWN):
            Y = np.einsum("opvg,gqyh,ocpi,ieqh,uvxy->ucxe", a1, b1, a2, b2, X)
        else:
            Y = np.einsum("opug,gqxh,ocvi,ieyh,uvxy->pcqe", a1, b1, a2, b2, X)
        ref = np.vdot(X, Y)
        assert abs(val - ref) < 1e-11 * abs(ref), name


def test_unsupported_order_is_refused(emu):
    rng = np.random.default_rng(15)
    l, r, w1, w2, c = _operands(rng, (UP, DOWN), False)
    h = _term(l, r, w2, w1, (DOWN, UP), (0, 0), c.shape)
    out = np.zeros(c.shape)
    assert emu.emu_heff_apply_ft(E.F64, C.byref(h), c.ctypes.data, out.ctypes.data) == E.MPSE_ERR_SHAPE


def test_one_leg_term_has_the_steps_of_the_two_layer_matvec(emu):
    """d_down == 1, both layers up and transposed, one MPO site: step for step plan_heff2 - which is why a one-term
    mpse_pcg_sum returns the bits of mpse_pcg(twolayer=1)."""
    rng = np.random.default_rng(16)
    l, r = _rand(rng, (6, 3, 3, 6), True), _rand(rng, (5, 4, 4, 5), True)
    w = _rand(rng, (3, 4, 4, 4), False)
    h = _term(l, r, w, w, (UP, UP), (1, 1), (6, 4, 1, 5))
    assert emu.emu_ft_steps_equal_heff2(E.C128, C.byref(h)) == 4
    c = _rand(rng, (6, 4, 1, 5), True)
    out = np.full(c.shape, np.nan, dtype=complex)
    assert emu.emu_heff_apply_ft(E.C128, C.byref(h), c.ctypes.data, out.ctypes.data) == 0
    ref = np.einsum("abcd,befg,cfhi,jgik,aej->dhk", l, w, w, r, c[:, :, 0, :])
    assert np.abs(out[:, :, 0, :] - ref).max() < 1e-11 * np.abs(ref).max()


@pytest.mark.parametrize("dom", ["L", "R"])
@pytest.mark.parametrize("bonds", [(5, 1, 1, 5), (1, 5, 5, 1), (4, 1, 2, 3), (1, 4, 3, 2)])
@pytest.mark.parametrize("name", list(TERMS))
def test_environment_with_uneven_mpo_bonds(emu, name, bonds, dom):
    """MPO bonds that grow in one layer and shrink in the other (wl1 > wr1 with wr2 > wl2 and the reverse): the middle
    intermediate of the right-to-left chain carries wl1 * wr2 channel pairs, that of the left-to-right chain wl2 * wr1.
    The emulation refuses (-1) a plan whose steps reach past the temporaries the executor allocates."""
    legs = TERMS[name]
    rng = np.random.default_rng(17)
    Dl, du, dv, Dr = 3, 2, 3, 4
    wl1, wr1, wl2, wr2 = bonds
    d1 = du if legs[0] == UP else dv
    d2 = du if legs[1] == UP else dv
    w1, w2 = _rand(rng, (wl1, d1, d1, wr1), False), _rand(rng, (wl2, d2, d2, wr2), False)
    x = _rand(rng, (Dl, du, dv, Dr), True)
    l, r = _rand(rng, (Dl, wl1, wl2, Dl), True), _rand(rng, (Dr, wr1, wr2, Dr), True)
    env = l if dom == "L" else r
    h = _term(l, r, w1, w2, legs, (0, 1), x.shape)
    ref = ref_env(dom, env, w1, w2, legs, (0, 1), x)
    out = np.full(ref.shape, np.nan, dtype=complex)
    assert emu.emu_env_update_ft(E.C128, 0 if dom == "L" else 1, C.byref(h), env.ctypes.data, E.C128, x.ctypes.data,
                                 out.ctypes.data) == 0
    assert np.abs(out - ref).max() < 1e-11 * np.abs(ref).max()
    if dom == "L":
        res = np.full(x.shape, np.nan, dtype=complex)
        assert emu.emu_heff_apply_ft(E.C128, C.byref(h), x.ctypes.data, res.ctypes.data) == 0
        ref2 = ref_apply(l, r, w1, w2, legs, (0, 1), x)
        assert np.abs(res - ref2).max() < 1e-11 * np.abs(ref2).max()
