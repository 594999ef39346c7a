"""The finite-temperature primitives on the device - two MPO layers on a centre with two physical legs:
mpse_heff_apply_ft, mpse_env_update_ft, mpse_site_factor_ft / mpse_diag_ft - against the tensordot chains of
tests/contract_refs.py, which state

    out[d, u', v', k] = sum L[a, b, c, d] C[a, u, v, j] (layer 1 on its leg) (layer 2 on its leg) R[j, g, i, k]

from include/mpsengine.h alone (W(trans = 0)[., x, y, .] maps leg[y] -> leg'[x], trans != 0 the transpose; layer 1 acts
first; b / g the bonds of layer 1, c / i those of layer 2) and are held against the host emulation of the plans by
tests/test_contract_refs_host.py.  MPO sites are dense, not symmetric, with four different bond extents, so that a
wrong transposition flag or a swapped layer bond changes every number.  Bound 1e-12 throughout, the one of the
one-layer contractions at tile-crossing sizes (tests/test_engine_gpu.py test_contractions_midsize_vs_oracle)."""
import ctypes as C

import numpy as np
import pytest

from renormalizer_amd import engine as E

import contract_refs as cr
from contract_refs import UP, DOWN, rand, relerr

pytestmark = pytest.mark.gpu

LEGS = {"M1": (UP, UP), "M2": (UP, DOWN), "M3": (DOWN, DOWN)}
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
KINDS = {"f64": (False, False), "c128": (True, True), "c128_real_env": (True, False)}       # (centre, environments)
BONDS = (2, 3, 4, 2)                                   # wl1, wr1, wl2, wr2
# (Dl, d_up, d_down, Dr), (wl1, wr1, wl2, wr2)
SHAPES = [
    ((37, 3, 5, 45), BONDS),          # ragged against the 64-wide tiles and the 16-deep K tiles
    ((70, 4, 3, 66), BONDS),          # more than one tile in every product
    ((1, 3, 2, 9), (1, 3, 1, 2)),     # left end of a chain
    ((9, 2, 3, 1), (2, 1, 4, 1)),     # right end
    ((12, 3, 1, 10), BONDS),          # d_down = 1
    ((10, 1, 4, 12), BONDS),          # d_up = 1
]


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def _operands(seed, shape, bonds, legs, cplx, cplx_env):
    rng = np.random.default_rng(seed)
    Dl, du, dv, Dr = shape
    wl1, wr1, wl2, wr2 = bonds
    d1 = du if legs[0] == UP else dv
    d2 = du if legs[1] == UP else dv
    w1, w2 = rand(rng, (wl1, d1, d1, wr1), False), rand(rng, (wl2, d2, d2, wr2), False)
    l, r = rand(rng, (Dl, wl1, wl2, Dl), cplx_env), rand(rng, (Dr, wr1, wr2, Dr), cplx_env)
    c = rand(rng, shape, cplx)
    return l, r, w1, w2, c


def _device_term(eng, l, r, w1, w2, legs, trans, shape):
    dev = eng.asdevice
    keep = [dev(w1), dev(w2), dev(l), dev(r)]
    return eng.ft_term(keep[0], keep[1], legs[0], legs[1], trans[0], trans[1], shape, keep[2], keep[3]), keep


# ---------------------------------------------------------------------------------------- B1: mpse_heff_apply_ft
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("trans", TRANS, ids=lambda t: f"t{t[0]}{t[1]}")
@pytest.mark.parametrize("name", list(LEGS))
def test_heff_apply_ft_vs_numpy(eng, name, trans, kind):
    legs = LEGS[name]
    cplx, cplx_env = KINDS[kind]
    for k, (shape, bonds) in enumerate(SHAPES):
        l, r, w1, w2, c = _operands(100 + k, shape, bonds, legs, cplx, cplx_env)
        term, keep = _device_term(eng, l, r, w1, w2, legs, trans, shape)
        out = eng.heff_apply_ft(term, eng.asdevice(c)).to_host()
        ref = cr.ref_apply_ft(l, r, w1, w2, legs, trans, c)
        err = relerr(out, ref)
        print(f"apply_ft {name} trans {trans} {kind} {shape} {bonds}: {err:.2e}")
        assert out.shape == ref.shape and err < 1e-12, (shape, bonds, err)


def test_heff_apply_ft_refuses_down_then_up(eng):
    """layer 1 on the down leg and layer 2 on the up leg: MPSE_ERR_SHAPE (such layers commute: the caller swaps them)"""
    shape, bonds = SHAPES[0]
    l, r, w1, w2, c = _operands(7, shape, bonds, (DOWN, UP), False, False)
    term, keep = _device_term(eng, l, r, w1, w2, (DOWN, UP), (0, 0), shape)
    dc = eng.asdevice(c)
    out = eng.zeros(shape)
    assert eng.lib.mpse_heff_apply_ft(eng.ctx, dc.code, C.byref(term), dc.ptr, out.ptr) == E.MPSE_ERR_SHAPE
    assert np.all(out.to_host() == 0.0)
    env_out = eng.zeros((shape[3], bonds[1], bonds[3], shape[3]))
    assert eng.lib.mpse_env_update_ft(eng.ctx, dc.code, E.DOMAIN_L, C.byref(term), keep[2].ptr, keep[2].code, dc.ptr,
                                      env_out.ptr) == E.MPSE_ERR_SHAPE


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_leg_term_is_heff_apply2_bitwise(eng, kind):
    """d_down = 1, both layers up, both transposed, one MPO site: the header promises mpse_heff_apply2 step by step"""
    cplx, cplx_env = KINDS[kind]
    rng = np.random.default_rng(9)
    for (Dl, d, Dr, wl, wr) in ((37, 3, 45, 3, 4), (70, 4, 66, 2, 3), (1, 3, 9, 1, 2)):
        w = rand(rng, (wl, d, d, wr), False)
        l, r = rand(rng, (Dl, wl, wl, Dl), cplx_env), rand(rng, (Dr, wr, wr, Dr), cplx_env)
        c = rand(rng, (Dl, d, 1, Dr), cplx)
        dev = eng.asdevice
        dw, dl, dr, dc = dev(w), dev(l), dev(r), dev(c)
        term = eng.ft_term(dw, dw, UP, UP, 1, 1, c.shape, dl, dr)
        out = eng.heff_apply_ft(term, dc).to_host()
        h = E.mpse_heff()
        h.nsite = 1
        dm = h.dims
        dm.Dl_bra = dm.Dl_ket = Dl
        dm.Dr_bra = dm.Dr_ket = Dr
        dm.d0, dm.d1, dm.danc, dm.wl, dm.wm, dm.wr = d, 1, 1, wl, 1, wr
        h.L, h.l_dtype, h.R, h.r_dtype = dl.ptr, dl.code, dr.ptr, dr.code
        h.W0, h.w_dtype = dw.ptr, dw.code
        out2 = eng.empty(c.shape, c.dtype)
        eng._check(eng.lib.mpse_heff_apply2(eng.ctx, dc.code, C.byref(h), dc.ptr, out2.ptr))
        assert np.array_equal(out, out2.to_host()), (Dl, d, Dr)
        ref = cr.ref_apply_ft(l, r, w, w, (UP, UP), (1, 1), c)
        assert relerr(out, ref) < 1e-12, (Dl, d, Dr)


# ---------------------------------------------------------------------------------------- B2: mpse_env_update_ft
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dom", ["L", "R"])
@pytest.mark.parametrize("trans", TRANS, ids=lambda t: f"t{t[0]}{t[1]}")
@pytest.mark.parametrize("name", list(LEGS))
def test_env_update_ft_vs_numpy(eng, name, trans, dom, kind):
    """output (ket bond, layer 1, layer 2, bra bond), bra = conj(X)"""
    legs = LEGS[name]
    cplx, cplx_env = KINDS[kind]
    for k, (shape, bonds) in enumerate(SHAPES):
        l, r, w1, w2, x = _operands(200 + k, shape, bonds, legs, cplx, cplx_env)
        term, keep = _device_term(eng, l, r, w1, w2, legs, trans, shape)
        env, denv = (l, keep[2]) if dom == "L" else (r, keep[3])
        out = eng.env_update_ft(term, dom, denv, eng.asdevice(x)).to_host()
        ref = cr.ref_env_ft(dom, env, w1, w2, legs, trans, x)
        err = relerr(out, ref)
        print(f"env_ft {dom} {name} trans {trans} {kind} {shape} {bonds}: {err:.2e}")
        assert out.shape == ref.shape and err < 1e-12, (shape, bonds, err)


@pytest.mark.parametrize("trans", TRANS, ids=lambda t: f"t{t[0]}{t[1]}")
@pytest.mark.parametrize("name", list(LEGS))
def test_env_update_ft_from_the_ones_sentinel(eng, name, trans):
    """the edge of a chain: the float64 all-ones environment (1, 1, 1, 1) with a complex site"""
    legs = LEGS[name]
    one = np.ones((1, 1, 1, 1))
    for dom, (shape, bonds) in (("L", SHAPES[2]), ("R", SHAPES[3])):
        _, _, w1, w2, x = _operands(300, shape, bonds, legs, True, False)
        dev = eng.asdevice
        dw1, dw2 = dev(w1), dev(w2)
        term = eng.ft_term(dw1, dw2, legs[0], legs[1], trans[0], trans[1], shape)
        done = dev(one)
        assert done.dtype == np.float64
        out = eng.env_update_ft(term, dom, done, dev(x)).to_host()
        ref = cr.ref_env_ft(dom, one, w1, w2, legs, trans, x)
        assert out.dtype == np.complex128 and out.shape == ref.shape
        assert relerr(out, ref) < 1e-12, (dom, shape)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("trans", TRANS, ids=lambda t: f"t{t[0]}{t[1]}")
@pytest.mark.parametrize("name", list(LEGS))
def test_functional_three_ways(eng, name, trans, kind):
    """<X| term |X> = vdot(X, apply(X)) = sum(update_L(L, X) * R) = sum(L * update_R(R, X)), the environments paired
    index by index: three device chains with different intermediates, equal to 1e-11 of the value's magnitude (sums
    of up to ~1e7 products of O(1) numbers with random signs: rounding stays near 1e-14 of the value)"""
    legs = LEGS[name]
    cplx, cplx_env = KINDS[kind]
    for k, (shape, bonds) in enumerate(SHAPES[:4]):
        l, r, w1, w2, x = _operands(400 + k, shape, bonds, legs, cplx, cplx_env)
        term, keep = _device_term(eng, l, r, w1, w2, legs, trans, shape)
        dx = eng.asdevice(x)
        v1 = np.vdot(x, eng.heff_apply_ft(term, dx).to_host())
        v2 = np.sum(eng.env_update_ft(term, "L", keep[2], dx).to_host() * r)
        v3 = np.sum(l * eng.env_update_ft(term, "R", keep[3], dx).to_host())
        vref = np.vdot(x, cr.ref_apply_ft(l, r, w1, w2, legs, trans, x))
        mag = abs(vref)
        print(f"functional {name} trans {trans} {kind} {shape}: {vref:.6g} dev {abs(v1 - vref) / mag:.2e} "
              f"{abs(v2 - vref) / mag:.2e} {abs(v3 - vref) / mag:.2e}")
        assert abs(v1 - v2) <= 1e-11 * mag and abs(v1 - v3) <= 1e-11 * mag and abs(v2 - v3) <= 1e-11 * mag, shape
        assert abs(v1 - vref) <= 1e-11 * mag, shape


# ---------------------------------------------------------------------------------------- B3: the diagonal
DIAG_SHAPES = [((3, 2, 3, 4), BONDS), ((9, 3, 4, 11), BONDS)]     # the second: factor tensor and diagonal span workgroups


@pytest.mark.parametrize("cr_", [False, True], ids=["Rreal", "Rcplx"])
@pytest.mark.parametrize("cl", [False, True], ids=["Lreal", "Lcplx"])
@pytest.mark.parametrize("trans", TRANS, ids=lambda t: f"t{t[0]}{t[1]}")
@pytest.mark.parametrize("name", list(LEGS))
def test_diag_ft_vs_numpy_dense_operator(eng, name, trans, cl, cr_):
    """mpse_site_factor_ft / mpse_diag_ft against Re diag of the dense operator built in NumPy (the reference applied to
    every unit vector), all four k_diag_ft<LC, RC> instantiations; weights, shift and accumulation as in
    tests/test_pcg_sum_gpu.py test_device_diagonal_of_a_term"""
    legs = LEGS[name]
    for k, (shape, bonds) in enumerate(DIAG_SHAPES):
        rng = np.random.default_rng(500 + k)
        Dl, du, dv, Dr = shape
        wl1, wr1, wl2, wr2 = bonds
        d1 = du if legs[0] == UP else dv
        d2 = du if legs[1] == UP else dv
        w1, w2 = rand(rng, (wl1, d1, d1, wr1), False), rand(rng, (wl2, d2, d2, wr2), False)
        l, r = rand(rng, (Dl, wl1, wl2, Dl), cl), rand(rng, (Dr, wr1, wr2, Dr), cr_)
        term, keep = _device_term(eng, l, r, w1, w2, legs, trans, shape)
        ref = np.real(np.diag(cr.dense_ft(l, r, w1, w2, legs, trans, shape)))
        fac = eng.site_factor_ft(term)
        assert fac.shape == (wl1, wl2, du, dv, wr1, wr2)
        d = eng.diag_ft_sum([term], [fac], [1.0], 0.0).to_host().ravel()
        err = np.abs(d - ref).max() / np.abs(ref).max()
        print(f"diag_ft {name} trans {trans} L{'c' if cl else 'r'} R{'c' if cr_ else 'r'} {shape}: {err:.2e}")
        assert err <= 1e-12, shape
        d2w = eng.diag_ft_sum([term, term], [fac, fac], [0.5, 2.0], 0.75).to_host().ravel()
        assert np.abs(d2w - (0.75 + 2.5 * ref)).max() <= 1e-12 * (0.75 + 2.5 * np.abs(ref).max()), shape
