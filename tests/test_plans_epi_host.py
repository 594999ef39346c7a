"""CPU check of the folded one-site matvec plan with the epilogue mix (mpse_plans.h: plan_heff1_fold(...,
mix_epilogue)): the plane of R's unit channel formed in the epilogue of the first product with R.  The plans run on host
memory through the naive executor of tests/host_emu (plan_emu_epi.cpp: its exports) against the dense contraction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from renormalizer_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_C, B_OUT, B_T1, B_T2, B_L, B_R = 4, 6, 7, 8, 0, 1
K_WMIX, K_GGEMM = 2, 3


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_epi") / "libplan_emu_epi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "plan_emu_epi.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_epi_apply.argtypes = [C.c_int, C.POINTER(E.mpse_heff), C.c_void_p, C.c_void_p, C.c_int,
                                  C.POINTER(C.c_longlong)]
    lib.emu_epi_steps.argtypes = [C.c_int, C.POINTER(E.mpse_heff), C.c_int, C.POINTER(C.c_longlong), C.c_longlong]
    lib.emu_epi_steps.restype = C.c_longlong
    return lib


def _band(rng, d, offsets):
    m = np.zeros((d, d))
    for o in offsets:
        m += np.diag(rng.standard_normal(d - abs(o)) + 3.0, o)      # (no entry of a band is zero: first and last rows too)
    return m


def _site(rng, d, kind, wr=4):
    """(wr + 1, d, d, wr) sites: channel 0 is L's unit channel, channel wr - 1 R's.  Channels 1, 2 (and 5 ... for wr > 4)
    pass through; the plane of R's unit channel receives what `kind` says."""
    w = np.zeros((wr + 1, d, d, wr))
    eye = np.eye(d)
    ru = wr - 1
    w[0, :, :, 0] = eye
    w[1, :, :, 1] = eye
    w[2, :, :, 2] = eye
    for f in range(3, ru):                  # further channels of R
        w[f + 2, :, :, f] = eye
    w[4, :, :, ru] = eye
    if kind == "ident":
        w[0, :, :, ru] = eye
    elif kind == "diag":
        w[0, :, :, ru] = _band(rng, d, (0,))
    elif kind == "tri":
        w[0, :, :, ru] = _band(rng, d, (0,))
        w[3, :, :, ru] = _band(rng, d, (-1, 1))
    elif kind in ("penta", "second", "many"):   # the Holstein phonon site: band(+-2) on the centre, a tridiagonal block
        w[0, :, :, ru] = _band(rng, d, (-2, 0, 2))
        w[3, :, :, ru] = _band(rng, d, (-1, 0, 1))
        if kind == "second":
            w[3, :, :, 1] = _band(rng, d, (-1, 1))      # a second mixed plane, at f != ru
    elif kind == "wide":
        w[0, :, :, ru] = _band(rng, d, (-3, 0))
    elif kind == "dense":
        w[0, :, :, ru] = _band(rng, d, (0,))
        w[3, :, :, ru] = rng.standard_normal((d, d))
    else:
        raise ValueError(kind)
    return w


def _heff(l, r, w0, c, lu, ru):
    h = E.mpse_heff()
    h.nsite, h.l_unit, h.r_unit = 1, lu, ru
    dm = h.dims
    dm.Dl_ket = dm.Dl_bra = c.shape[0]
    dm.Dr_ket = dm.Dr_bra = c.shape[2]
    dm.danc, dm.wl, dm.wr, dm.d0, dm.d1, dm.wm = 1, w0.shape[0], w0.shape[3], w0.shape[1], 1, 1
    keep = [np.ascontiguousarray(x) for x in (l, r, w0, c)]
    h.L, h.l_dtype = keep[0].ctypes.data, E.dtype_code(keep[0].dtype)
    h.R, h.r_dtype = keep[1].ctypes.data, E.dtype_code(keep[1].dtype)
    h.W0, h.w_dtype = keep[2].ctypes.data, E.F64
    return h, keep


def _operands(rng, D, d, w0, cplx, r_unit=True):
    wl, wr = w0.shape[0], w0.shape[3]

    def rand(shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if cplx else a
    l, r, c = rand((D, wl, D)), rand((D, wr, D)), rand((D, d, D))
    l[:, 0, :] = np.eye(D)
    if r_unit:
        r[:, wr - 1, :] = np.eye(D)
    return l, r, c


def _apply(emu, l, r, w0, c, r_unit, mix):
    h, keep = _heff(l, r, w0, c, 1, w0.shape[3] if r_unit else 0)
    out = np.full(c.shape, np.nan, dtype=c.dtype)
    info = (C.c_longlong * 8)()
    st = emu.emu_epi_apply(E.C128 if np.iscomplexobj(c) else E.F64, C.byref(h), keep[3].ctypes.data, out.ctypes.data,
                           1 if mix else 0, info)
    assert st == 0
    return out, dict(steps=info[0], wmix_steps=info[1], wmix_dsts=info[2], mix_first=info[3], mix_later=info[4],
                     r_steps=info[5], two=info[6], t1=info[7])


# (kind, D, d, wr, R's unit channel known, terms the first product with R carries (0: the elementwise pass stays),
#  K_WMIX destinations left)
CASES = [
    ("ident", 8, 4, 4, True, 2, 0),       # two identity blocks: the centre and `out` itself (written by the product with L)
    ("diag", 12, 4, 4, True, 2, 0),
    ("tri", 8, 8, 4, True, 4, 0),
    ("penta", 16, 4, 4, True, 7, 0),      # D d = 64: halved tiles for the complex centre
    ("penta", 8, 16, 4, True, 7, 0),
    ("penta", 12, 8, 4, True, 7, 0),
    ("second", 8, 8, 4, True, 7, 1),      # K_WMIX stays for the plane at f != ru only
    ("many", 8, 4, 7, True, 7, 0),        # six products with R in two launches: the first carries the mix
    ("dense", 8, 8, 4, True, 0, 1),
    ("wide", 8, 8, 4, True, 0, 1),        # half-bandwidth 3
    ("penta", 8, 12, 4, True, 0, 1),      # 64 % 12 != 0
    ("penta", 8, 8, 4, False, 0, 1),      # R without a unit channel: no plane is `out`
]


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("kind,D,d,wr,r_unit,nmix,ndst", CASES)
def test_epilogue_mix_plan_vs_dense(emu, kind, D, d, wr, r_unit, nmix, ndst, cplx):
    rng = np.random.default_rng(5)
    w0 = _site(rng, d, kind, wr)
    l, r, c = _operands(rng, D, d, w0, cplx, r_unit)
    ref = np.einsum("abc,bdef,lfk,cek->adl", l, w0, r, c)
    bound = 1e-12 * np.abs(ref).max() * D * 5          # sums of <= 5 D d products of O(1) numbers in double precision
    out, info = _apply(emu, l, r, w0, c, r_unit, True)
    assert np.abs(out - ref).max() < bound
    assert info["mix_first"] == nmix and info["mix_later"] == 0
    assert info["wmix_dsts"] == ndst and info["wmix_steps"] == (1 if ndst else 0)
    assert info["r_steps"] == (2 if kind == "many" else 1)
    assert info["two"] == (1 if cplx and (D * d) % 64 == 0 else 0)
    # the same site without the parameter: one elementwise pass forms the plane
    out0, info0 = _apply(emu, l, r, w0, c, r_unit, False)
    assert np.abs(out0 - ref).max() < bound
    assert info0["mix_first"] == 0 and info0["mix_later"] == 0 and info0["wmix_steps"] == 1
    if nmix:
        # the identity block's product goes straight into `out`: one temporary plane less
        assert info["t1"] == info0["t1"] - D * d * D


def test_zero_centre_gives_exact_zero(emu):
    rng = np.random.default_rng(6)
    w0 = _site(rng, 8, "penta")
    l, r, c = _operands(rng, 8, 8, w0, True)
    out, info = _apply(emu, l, r, w0, 0 * c, True, True)
    assert info["mix_first"] == 7 and not out.any()


def _steps(emu, h, which):
    rec = (C.c_longlong * 4096)()
    n = emu.emu_epi_steps(E.C128, C.byref(h), which, rec, 4096)
    assert n > 0
    return list(rec[:n])


def test_parameter_off_is_todays_plan(emu):
    """Without the parameter, and with it off, the step list is the one the plan had before the epilogue mix: kinds,
    buffers, offsets (written out here for the Holstein phonon site)."""
    rng = np.random.default_rng(7)
    D, d = 16, 4
    w0 = _site(rng, d, "penta")
    l, r, c = _operands(rng, D, d, w0, True)
    h, keep = _heff(l, r, w0, c, 1, 4)
    plane = D * d * D
    today = [1, 2 * plane, 2 * plane,
             -1, K_GGEMM,
             -2, B_T2, 0, 0, 0, 1, 0, B_L, 1 * D, B_C, 0,              # channels 1, 2: their planes
             -2, B_T2, plane, 0, 0, 1, 0, B_L, 2 * D, B_C, 0,
             -2, B_T1, 0, 0, 0, 1, 0, B_L, 3 * D, B_C, 0,              # channels 3, 4: temporaries
             -2, B_T1, plane, 0, 0, 1, 0, B_L, 4 * D, B_C, 0,
             -1, K_WMIX,
             -3, B_OUT, 0, 3, B_C, 0, 0, 3, 0, B_T1, 0, 3, 3, 0, B_T1, plane, 4, 3, 1,
             -1, K_GGEMM,
             -2, B_OUT, 0, 1, 1, 3, 0, B_C, 0, B_R, 0, B_T2, 0, B_R, D, B_T2, plane, B_R, 2 * D]
    assert _steps(emu, h, 0) == today
    assert _steps(emu, h, 1) == today
    on = _steps(emu, h, 2)
    assert on != today and K_WMIX not in [on[i + 1] for i, v in enumerate(on) if v == -1]
    for kind, dd in (("second", 8), ("dense", 8), ("many", 4), ("penta", 12)):
        w1 = _site(rng, dd, kind, 7 if kind == "many" else 4)
        l, r, c = _operands(rng, 8, dd, w1, True)
        h, keep = _heff(l, r, w1, c, 1, w1.shape[3])
        assert _steps(emu, h, 0) == _steps(emu, h, 1)
