"""The identity ("unit") channel of an environment on the device, from detection to use.

mpse_env_unit_channel (k_unit_deviation) against its definition; then mpse_heff_apply and mpse_env_update, called through
the C entry points alone (no MPO-site description, no solver: the small-centre kernel, the fused kernel and the folded
plan stay out), at shapes whose unit slice costs at least 2^27 multiply-adds, so that the plans replace that slice by a
copy and, on the R side of a matvec, read it as the beta source of the first product (GemmArgs::Cin in the epilogues of
k_gemm and in k_splitk_reduce).  References are the tensordot chains of tests/contract_refs.py in float64 / complex128,
held against the host emulation of the plans by tests/test_contract_refs_host.py.

Which path ran is read from the counters the engine has:
  * launches (mpse_gemm_path_stats): a unit channel strictly inside splits its side into two products, one launch more
    than the same call with the unit fields zeroed; a unit channel at the first or last index leaves the number
    unchanged; with w = 1 no product is left on that side, one launch fewer;
  * the algorithmic flops of the timed launches (mpse_prof_get with every launch timed) fall by exactly the flops of
    the slice that became a copy - this also tells the shortcut from the plain path when the unit channel is first or
    last;
  * general / split_b1 where a case is meant to reach the general kernel or split-K.
Bounds: 1e-12 against the reference (test_contractions_midsize_vs_oracle), 1e-13 between the two device paths of one
operation (test_env_update_described_site_elementwise_mpo_step), two runs of one call bitwise equal."""
import ctypes as C
import zlib

import numpy as np
import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.mps.lib import UNIT_TOL

import contract_refs as cr
from contract_refs import rand, relerr
from gemm_policy import plain_plan

pytestmark = pytest.mark.gpu


def _seed(*names):
    return zlib.crc32("/".join(names).encode())


THRESHOLD = 1 << 27          # multiply-adds of a slice from which the plans skip it (mpse_plans.h unit_threshold)
assert UNIT_TOL == 1e-12


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


# ====================================================================================== A1: detection
def _chan_dev(env, b):
    """max |env[:, b, :] - I|; NaN stays NaN (and never compares <= tol)"""
    return np.abs(env[:, b, :] - np.eye(env.shape[0])).max()


def _first_unit(devs, tol):
    for b, v in enumerate(devs):
        if v <= tol:
            return b + 1
    return 0


def _detect(eng, dev_env, tol=UNIT_TOL):
    out = C.c_int64(-1)
    D, w = dev_env.shape[0], dev_env.shape[1]
    eng._check(eng.lib.mpse_env_unit_channel(eng.ctx, dev_env.code, dev_env.ptr, D, w, tol, C.byref(out)))
    return out.value


def _poke(eng, dev_env, index, value):
    """dev_env[index] = value on the device (one element)"""
    flat = int(np.ravel_multi_index(index, dev_env.shape))
    v = np.array([value], dtype=dev_env.dtype)
    eng._check(eng.lib.mpse_memcpy_h2d(eng.ctx, dev_env.ptr + flat * dev_env.dtype.itemsize, v.ctypes.data, v.nbytes))


def _env_with_units(rng, D, w, units, cplx):
    env = rand(rng, (D, w, D), cplx)
    for u in units:
        env[:, u, :] = np.eye(D)
    return env


DET_D = (1, 5, 64, 65, 255, 256, 257, 600)
DET_W = (1, 3, 7)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("w", DET_W)
@pytest.mark.parametrize("D", DET_D)
def test_detection_positions(eng, D, w, cplx):
    """an exact identity in the first, a middle and the last channel, two of them (the first wins), none"""
    rng = np.random.default_rng(1000 * D + 10 * w + cplx)
    configs = [(), (0,), (w // 2,), (w - 1,)]
    if w > 1:
        configs.append((w // 2, w - 1))
        configs.append((0, w - 1))
    for units in configs:
        env = _env_with_units(rng, D, w, units, cplx)
        ref = _first_unit([_chan_dev(env, b) for b in range(w)], UNIT_TOL)
        assert ref == (min(units) + 1 if units else 0)          # (random channels are nowhere near the identity)
        assert _detect(eng, eng.asdevice(env)) == ref, (D, w, units)


def _placements(D, cplx):
    """(row, column, part) of the single elements that get perturbed"""
    p = {(0, 0), (D - 1, D - 1), (0, D - 1), (D - 1, 0)}
    for col in (63, 64, 256):
        if col < D:
            p.add((min(1, D - 1), col))
            p.add((D - 1, col))
    out = [(a, c, "re") for a, c in sorted(p)]
    if cplx:
        out += [(0, 0, "im"), (D - 1, D - 1, "im"), (D // 2, D // 2, "im")]
    return out


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("w", DET_W)
@pytest.mark.parametrize("D", DET_D)
def test_detection_single_element_perturbations(eng, D, w, cplx):
    """one element of the identity channel off by 2 tol hides the channel, by tol / 2 does not: diagonal and off-diagonal
    corners, columns on both sides of a wave edge and of the 256-stride loop, the imaginary part of a diagonal element"""
    rng = np.random.default_rng(2000 * D + 10 * w + cplx)
    for u in sorted({0, w // 2, w - 1}):
        env = _env_with_units(rng, D, w, (u,), cplx)
        dev = eng.asdevice(env)
        devs = [_chan_dev(env, b) for b in range(w)]
        assert _detect(eng, dev) == u + 1
        for (a, c, part) in _placements(D, cplx):
            base = env[a, u, c]
            for sign in (1.0, -1.0):
                for eps, hidden in ((2 * UNIT_TOL, True), (0.5 * UNIT_TOL, False)):
                    val = base + (sign * eps * 1j if part == "im" else sign * eps)
                    env[a, u, c] = val
                    d2 = list(devs)
                    d2[u] = _chan_dev(env, u)
                    env[a, u, c] = base
                    ref = _first_unit(d2, UNIT_TOL)
                    assert ref == (0 if hidden else u + 1), (D, w, u, a, c, part, eps, d2[u])
                    _poke(eng, dev, (a, u, c), val)
                    got = _detect(eng, dev)
                    _poke(eng, dev, (a, u, c), base)
                    assert got == ref, (D, w, u, a, c, part, sign * eps)
        assert _detect(eng, dev) == u + 1                        # (every element put back)


def _non_finite(base, cplx):
    """`base` with NaN / inf in its real part, its imaginary part, or both"""
    if not cplx:
        return [np.nan, np.inf, -np.inf]
    re, im = base.real, base.imag
    return [complex(np.nan, im), complex(re, np.nan), complex(np.nan, np.nan), complex(np.inf, im), complex(re, -np.inf)]


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("D", DET_D)
def test_detection_non_finite(eng, D, cplx):
    """NaN or inf anywhere inside a channel: not a unit channel - in either part of a complex element, the other part
    staying what the identity has there; the same values in another channel do not hide a unit channel"""
    w = 3
    rng = np.random.default_rng(3000 * D + cplx)
    for u in range(w):
        env = _env_with_units(rng, D, w, (u,), cplx)
        dev = eng.asdevice(env)
        o = (u + 1) % w
        for (a, c) in sorted({(0, 0), (D - 1, D - 1), (0, D - 1), (D // 2, min(D - 1, 64)), (D - 1, D // 2)}):
            base = env[a, u, c]
            for v in _non_finite(base, cplx):
                env[a, u, c] = v
                ref = _first_unit([_chan_dev(env, b) for b in (u,)], UNIT_TOL)
                env[a, u, c] = base
                assert ref == 0
                _poke(eng, dev, (a, u, c), v)
                got = _detect(eng, dev)
                _poke(eng, dev, (a, u, c), base)
                assert got == 0, (D, u, a, c, v)
            for v in _non_finite(env[a, o, c], cplx):
                _poke(eng, dev, (a, o, c), v)
                got = _detect(eng, dev)
                _poke(eng, dev, (a, o, c), env[a, o, c])
                assert got == u + 1, (D, u, o, a, c, v)
        assert _detect(eng, dev) == u + 1


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("w", [1024, 1025, 2048, 2049])
def test_detection_many_channels(eng, w, cplx):
    """D = 2 with w on both sides of the two read-back paths (up to 1024 channels through the published slot, above
    through a copy), the largest w served, and w = 2049, which answers 0 without device work"""
    rng = np.random.default_rng(w + cplx)
    for units in ((), (0,), (w // 2,), (w - 1,), (w - 2, w - 1)):
        env = _env_with_units(rng, 2, w, units, cplx)
        ref = _first_unit([_chan_dev(env, b) for b in range(w)], UNIT_TOL)
        assert ref == (min(units) + 1 if units else 0)
        dev = eng.asdevice(env)
        assert _detect(eng, dev) == (ref if w <= 2048 else 0), (w, units)
    # the last channel, hidden by 2 tol on its last element and not by tol / 2
    u = w - 1
    dev = eng.asdevice(_env_with_units(rng, 2, w, (u,), cplx))
    for eps, hidden in ((2 * UNIT_TOL, True), (0.5 * UNIT_TOL, False)):
        _poke(eng, dev, (1, u, 1), 1.0 + eps)
        assert _detect(eng, dev) == (0 if (hidden or w > 2048) else u + 1), (w, eps)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_detection_scratch_reuse(eng, cplx):
    """seven channels without a unit channel, then three with one: the deviations of the first call do not linger"""
    rng = np.random.default_rng(77)
    for D in (5, 257):
        first = eng.asdevice(_env_with_units(rng, D, 7, (), cplx))
        second = eng.asdevice(_env_with_units(rng, D, 3, (2,), cplx))
        third = eng.asdevice(_env_with_units(rng, D, 7, (6,), cplx))
        assert _detect(eng, first) == 0
        assert _detect(eng, second) == 3
        assert _detect(eng, third) == 7
        assert _detect(eng, first) == 0


# ====================================================================================== shared: evidence of the path
class Evidence:
    """counters around one call: path counters of the contraction kernel and the algorithmic flops of its launches (every
    launch timed while the block is open)"""
    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        eng = self.eng
        eng.prof_enable(1)
        eng.prof_reset()
        self.p0 = eng.gemm_path_stats()
        return self

    def __exit__(self, *exc):
        eng = self.eng
        try:
            if exc[0] is None:
                p1 = eng.gemm_path_stats()
                self.paths = {k: p1[k] - self.p0[k] for k in p1}
                prof = eng.prof_get()
                self.flops = sum(prof[v]["flops"] for v in ("f64xf64", "c128xf64", "f64xc128", "c128xc128"))
                self.timed = sum(prof[v]["launches"] for v in ("f64xf64", "c128xf64", "f64xc128", "c128xc128"))
        finally:
            eng.prof_enable(0)
        return False


def _flops_per_mac(code_a, code_b):
    """algorithmic real flops per multiply-add of a product (include/mpsengine.h, mpse_prof_get)"""
    return {0: 2.0, 1: 4.0, 2: 8.0}[int(code_a == E.C128) + int(code_b == E.C128)]


def _sectors(D):
    """two bond sectors whose edge is no multiple of 64 (nor of 16)"""
    n0 = (D * 25) // 64 + 1
    n0 += n0 % 16 == 0
    return np.array([0] * n0 + [1] * (D - n0))


_CHARGE = np.array([0, 1, -1, 0, 0, 1, -1])


def _sparse_env(rng, Db, w, Dk, cplx, unit=None):
    """block-sparse environment: channel b carries the charge _CHARGE[b]; the identity written into channel `unit`"""
    sb, sk = _sectors(Db), _sectors(Dk)
    e = rand(rng, (Db, w, Dk), cplx) * (sb[:, None, None] - sk[None, None, :] == _CHARGE[None, :w, None])
    if unit is not None:
        assert Db == Dk
        e[:, unit, :] = np.eye(Db)
    return e


def _sparse_centre(rng, shape, cplx):
    sl, sr = _sectors(shape[0]), _sectors(shape[-1])
    mask = (sl[:, None] == sr[None, :]).reshape((shape[0],) + (1,) * (len(shape) - 2) + (shape[-1],))
    return rand(rng, shape, cplx) * mask


DTYPES = {"f64": (False, False), "c128": (True, True), "c128_real_env": (True, False)}     # (centre, environments)


# ====================================================================================== A2: mpse_heff_apply
class HeffCase:
    """operands of one matvec on the device and its slices: `phys` the physical / ancilla extents of the centre in
    memory order, `anc` (danc, danc1) where the centre has ancilla legs"""
    def __init__(self, eng, nsite, Dl, phys, Dr, wbonds, kind, pos, seed, anc=None, bra_bonds=None):
        self.eng, self.nsite = eng, nsite
        cplx, cplx_env = DTYPES[kind]
        rng = np.random.default_rng(seed)
        wl, wr = wbonds[0], wbonds[-1]
        Dlb, Drb = bra_bonds if bra_bonds else (Dl, Dr)
        self.ul = {"first": 0, "mid": wl // 2, "last": wl - 1}[pos]
        self.ur = {"first": 0, "mid": wr // 2, "last": wr - 1}[pos]
        square = bra_bonds is None
        self.l = _sparse_env(rng, Dlb, wl, Dl, cplx_env, self.ul if square else None)
        self.r = _sparse_env(rng, Drb, wr, Dr, cplx_env, self.ur if square else None)
        if nsite == 0:
            self.ws = []
        elif nsite == 1:
            self.ws = [rand(rng, (wl, phys[0], phys[0], wr), False)]
        else:
            d0, d1 = (phys[0], phys[2]) if anc else phys
            self.ws = [rand(rng, (wl, d0, d0, wbonds[1]), False), rand(rng, (wbonds[1], d1, d1, wr), False)]
        self.c = _sparse_centre(rng, (Dl,) + tuple(phys) + (Dr,), cplx)
        self.oshape = (Dlb,) + tuple(phys) + (Drb,)
        dev = eng.asdevice
        self.dl, self.dr, self.dc = dev(self.l), dev(self.r), dev(self.c)
        self.dw = [dev(w) for w in self.ws]
        h = self.h = E.mpse_heff()
        h.nsite = nsite
        d = h.dims
        d.Dl_bra, d.Dl_ket, d.Dr_bra, d.Dr_ket = Dlb, Dl, Drb, Dr
        d.wl, d.wr = wl, wr
        d.wm = wbonds[1] if nsite == 2 else 1
        d.d0 = phys[0] if nsite >= 1 else 1
        d.d1 = (phys[2] if anc else phys[1]) if nsite == 2 else 1
        d.danc, d.danc1 = (anc if anc else (1, 0))
        h.L, h.l_dtype, h.R, h.r_dtype = self.dl.ptr, self.dl.code, self.dr.ptr, self.dr.code
        if nsite >= 1:
            h.W0, h.w_dtype = self.dw[0].ptr, self.dw[0].code
        if nsite == 2:
            h.W1 = self.dw[1].ptr
        n_mid = int(np.prod(phys)) if phys else 1
        # multiply-adds of the slice of one channel on either side (the products L[:, b, :] . C and T[.., f, ..] . R[:, f, :]^T)
        self.macs_l = Dlb * Dl * n_mid * Dr
        self.macs_r = Dlb * n_mid * Dr * Drb
        self.flops_l = self.macs_l * _flops_per_mac(self.dl.code, self.dc.code)
        self.flops_r = self.macs_r * _flops_per_mac(self.dc.code, self.dr.code)
        self.wl, self.wr = wl, wr

    def reference(self):
        return cr.ref_heff(self.l, self.r, self.ws, self.c)

    def run(self, lu, ru, evidence=True):
        eng = self.eng
        self.h.l_unit, self.h.r_unit = lu, ru
        out = eng.empty(self.oshape, self.c.dtype)
        if not evidence:
            eng._check(eng.lib.mpse_heff_apply(eng.ctx, out.code, C.byref(self.h), self.dc.ptr, out.ptr))
            return out.to_host(), None
        with Evidence(eng) as ev:
            eng._check(eng.lib.mpse_heff_apply(eng.ctx, out.code, C.byref(self.h), self.dc.ptr, out.ptr))
        return out.to_host(), ev


def _launch_delta(w, u):
    """launches of one side with the unit channel u of w skipped, minus those of the plain product"""
    return -1 if w == 1 else (1 if 0 < u < w - 1 else 0)


def _check_heff_case(case, name, sides=("L", "R", "both"), expect_shortcut=True, general=None, unsplit=False):
    assert not expect_shortcut or min(case.macs_l, case.macs_r) >= THRESHOLD, (name, case.macs_l, case.macs_r)
    ref = case.reference()
    plain, ev0 = case.run(0, 0)
    e0 = relerr(plain, ref)
    print(f"{name}: plain err {e0:.2e} launches {ev0.paths['launches']} general {ev0.paths['general']} "
          f"split_b1 {ev0.paths['split_b1']} flops {ev0.flops:.4g}")
    assert e0 < 1e-12, name
    assert ev0.timed == ev0.paths["launches"]              # every launch of the kernel was timed: the flops are complete
    assert not unsplit or ev0.paths["split_b1"] == 0, f"{name}: meant to run unsplit"
    for side in sides:
        lu = case.ul + 1 if side in ("L", "both") else 0
        ru = case.ur + 1 if side in ("R", "both") else 0
        out, ev = case.run(lu, ru)
        again, _ = case.run(lu, ru, evidence=False)
        e1, e2 = relerr(out, ref), relerr(out, plain)
        dl = ev.paths["launches"] - ev0.paths["launches"]
        df = ev0.flops - ev.flops
        print(f"{name} {side} (l_unit {lu}, r_unit {ru}): err {e1:.2e} vs plain {e2:.2e} launches {dl:+d} "
              f"general {ev.paths['general']} split_b1 {ev.paths['split_b1']} flops saved {df:.6g}")
        assert e1 < 1e-12, (name, side)
        assert e2 < 1e-13, (name, side)
        assert np.array_equal(out, again), (name, side)
        want_dl = want_df = 0
        if expect_shortcut:
            if lu:
                want_dl += _launch_delta(case.wl, case.ul)
                want_df += case.flops_l
            if ru:
                want_dl += _launch_delta(case.wr, case.ur)
                want_df += case.flops_r
        assert ev.timed == ev.paths["launches"]
        assert dl == want_dl, f"{name} {side}: {dl:+d} launches against the plain plan, expected {want_dl:+d}"
        assert df == want_df, f"{name} {side}: {df} flops saved, expected {want_df} (shortcut {'not ' if df == 0 else ''}taken)"
        if general is not None:
            assert ev.paths["general"] == general, (name, side, ev.paths["general"])
        if unsplit:     # no reduction launch: the beta source was read by the epilogue of k_gemm
            assert ev.paths["split_b1"] == 0 and ev.paths["split_batched"] == 0, f"{name} {side}: meant to run unsplit"
    return ref


# name: (nsite, Dl, phys, Dr, MPO bonds, ancilla extents)
HEFF_SHAPES = {
    "bond512": (0, 512, (), 512, (3,), None),
    "bond520": (0, 520, (), 520, (3,), None),
    "site320": (1, 320, (5,), 320, (3, 4), None),
    "site328x324": (1, 328, (5,), 324, (5, 3), None),
    "mpdm208": (1, 208, (4, 4), 208, (4, 4), (4, 0)),
    "two212x204": (2, 212, (4, 4), 204, (3, 4, 3), None),
    # many output tiles (63 x 5 and 65 x 5): on up to 315 compute units the products with R run unsplit, so the beta
    # source is read by the epilogue of k_gemm itself - the three epilogue forms are the three dtype kinds - where the
    # shapes above, with fewer tiles than compute units, all leave it to the reduction kernel of split-K
    "site250x260_d16": (1, 250, (16,), 260, (3, 4), None),
    "mpdm130x260_d8": (1, 130, (8, 4), 260, (4, 4), (4, 0)),
}
UNSPLIT = ("site250x260_d16", "mpdm130x260_d8")


@pytest.mark.parametrize("pos", ["first", "mid", "last"])
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("shape", list(HEFF_SHAPES))
def test_heff_apply_unit_channels(eng, shape, kind, pos):
    """every shape crosses the threshold on both sides; the unit channel first, inside and last, on L only, R only and
    both.  The unit channel inside splits its side into two products, of which the first carries the beta source on
    the R side."""
    nsite, Dl, phys, Dr, wb, anc = HEFF_SHAPES[shape]
    case = HeffCase(eng, nsite, Dl, phys, Dr, wb, kind, pos, seed=_seed(shape, kind, pos), anc=anc)
    general = None
    unsplit = shape in UNSPLIT
    if unsplit:
        cplx, cplx_env = DTYPES[kind]
        rows = Dl * int(np.prod(phys))
        for nf in range(1, wb[-1] + 1):
            plan = plain_plan(eng.n_cu, rows, Dr, nf * Dr, 1, ca=cplx, cb=cplx_env, beta=True)
            assert plan["ksplit"] == 1, f"{shape}: a product with R over {nf} channels splits on {eng.n_cu} compute units"
    if shape == "mpdm130x260_d8":
        # as below, but the MPO step of this site (wl d = 32) is a batched product with a two-level K index of its own
        general = 2
    if shape == "mpdm208":
        # The K index of a product with R is (channels | ket bond) with the ancilla between them: two levels, the
        # general kernel, as soon as it spans two channels - the plain product (4), the only product beside a unit
        # channel at the edge (3), and the FIRST product beside the unit channel inside (wr // 2 = 2 channels, then 1):
        # the one that reads the beta source through the two-level row map.  The MPO step of a site with wl d = d wr =
        # 16 runs as an elementwise kernel and the products with L have a plain K index: exactly one general launch.
        general = 1
    _check_heff_case(case, f"{shape}/{kind}/{pos}", general=general, unsplit=unsplit)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_heff_apply_single_channel_is_a_copy(eng, kind):
    """0-site, w = 1, the only channel the identity: a copy and no product on that side"""
    case = HeffCase(eng, 0, 512, (), 512, (1,), kind, "first", seed=5)
    ref = _check_heff_case(case, f"bond512_w1/{kind}")
    assert np.array_equal(ref, case.c) or relerr(ref, case.c) < 1e-15       # H = 1 x 1: the result is the centre
    out, ev = case.run(1, 1)
    assert ev.paths["launches"] == 0 and ev.flops == 0
    assert np.array_equal(out, case.c)


def _skinny_dr(n_cu, Dl, d, w, ca, cb):
    """the smallest right bond from 1024 on (where the slice of one channel reaches the threshold) at which the launch
    policy splits every product with R of the skinny centre along K"""
    for Dr in (1024, 1088, 1152, 1280, 1536, 2048):
        if Dl * d * Dr * Dr < THRESHOLD:
            continue
        if all(plain_plan(n_cu, Dl * d, Dr, nf * Dr, 1, ca=ca, cb=cb, beta=True)["ksplit"] > 1 for nf in range(1, w + 1)):
            return Dr
    raise AssertionError(f"({Dl}, {d}, Dr): no right bond in 1024..2048 whose products with R split on {n_cu} compute units")


@pytest.mark.parametrize("pos", ["first", "mid", "last"])
@pytest.mark.parametrize("kind", list(DTYPES))
def test_heff_apply_beta_source_through_split_k(eng, kind, pos):
    """skinny result (64 x 2 rows, few output tiles): the products with R run split-K, so the slice of R's unit channel
    is added by the reduction kernel (k_splitk_reduce reads the beta source)"""
    Dl, d, w = 64, 2, 3
    cplx, cplx_env = DTYPES[kind]
    Dr = _skinny_dr(eng.n_cu, Dl, d, w, cplx, cplx_env)
    case = HeffCase(eng, 1, Dl, (d,), Dr, (w, w), kind, pos, seed=11 + len(kind))
    name = f"skinny({Dl},{d},{Dr})/{kind}/{pos}"
    assert case.macs_r >= THRESHOLD > case.macs_l, name
    ref = case.reference()
    plain, ev0 = case.run(0, 0)
    out, ev = case.run(0, case.ur + 1)
    again, _ = case.run(0, case.ur + 1, evidence=False)
    n_r = 2 if pos == "mid" else 1                              # products with R beside the unit channel
    print(f"{name}: err {relerr(out, ref):.2e} vs plain {relerr(out, plain):.2e} launches {ev0.paths['launches']} -> "
          f"{ev.paths['launches']} split_b1 {ev0.paths['split_b1']} -> {ev.paths['split_b1']} "
          f"flops saved {ev0.flops - ev.flops:.6g}")
    assert relerr(plain, ref) < 1e-12 and relerr(out, ref) < 1e-12, name
    assert relerr(out, plain) < 1e-13, name
    assert np.array_equal(out, again), name
    assert ev.paths["launches"] - ev0.paths["launches"] == n_r - 1, name
    assert ev0.flops - ev.flops == case.flops_r, f"{name}: the shortcut did not run"
    # The launches are the product with L and those with R (the MPO step of a d = 2 site is an elementwise kernel):
    # every product with R was split, the one that carries the beta source among them
    l_split = int(plain_plan(eng.n_cu, w * Dl, d * Dr, Dl, 1, ca=cplx_env, cb=cplx)["ksplit"] > 1)
    assert ev.paths["launches"] == 1 + n_r and ev0.paths["launches"] == 2, name
    assert ev0.paths["split_b1"] == l_split + 1, f"{name}: the plain product with R ran unsplit"
    assert ev.paths["split_b1"] == l_split + n_r, f"{name}: a product with R ran unsplit"
    # the unit on the small L side is ignored: below the threshold there
    out_l, ev_l = case.run(case.ul + 1, case.ur + 1)
    assert np.array_equal(out_l, out) and ev_l.flops == ev.flops, name


@pytest.mark.parametrize("kind", list(DTYPES))
def test_heff_apply_below_threshold_keeps_the_products(eng, kind):
    """just below the threshold on both sides the unit fields change nothing: the plain products run"""
    case = HeffCase(eng, 1, 288, (5,), 288, (3, 4), kind, "mid", seed=13)
    assert max(case.macs_l, case.macs_r) < THRESHOLD
    _check_heff_case(case, f"site288/{kind}", expect_shortcut=False)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_heff_apply_rectangular_ignores_units(eng, kind):
    """bra bonds != ket bonds (slices above the threshold): no channel of such an environment is a square identity,
    the unit fields must be ignored"""
    case = HeffCase(eng, 1, 340, (5,), 340, (3, 4), kind, "mid", seed=17, bra_bonds=(300, 300))
    assert min(case.macs_l, case.macs_r) >= THRESHOLD
    _check_heff_case(case, f"rect300x340/{kind}", expect_shortcut=False)


# ====================================================================================== A3: mpse_env_update
class EnvCase:
    def __init__(self, eng, dom, Dl, phys, Dr, wbonds, kind, pos, seed, bra_bonds=None):
        self.eng, self.dom = eng, dom
        cplx, cplx_env = DTYPES[kind]
        rng = np.random.default_rng(seed)
        wl, wr = wbonds
        d = phys[0]
        anc = phys[1] if len(phys) == 2 else 1
        Dlb, Drb = bra_bonds if bra_bonds else (Dl, Dr)
        we = wl if dom == "L" else wr
        Db, Dk = (Dlb, Dl) if dom == "L" else (Drb, Dr)
        self.u = {"first": 0, "mid": we // 2, "last": we - 1}[pos]
        self.we = we
        self.env = _sparse_env(rng, Db, we, Dk, cplx_env, self.u if bra_bonds is None else None)
        self.w = rand(rng, (wl, d, d, wr), False)
        self.ket = _sparse_centre(rng, (Dl,) + tuple(phys) + (Dr,), cplx)
        self.bra = _sparse_centre(rng, (Dlb,) + tuple(phys) + (Drb,), cplx)
        self.separate_only = bra_bonds is not None
        dev = eng.asdevice
        self.denv, self.dw, self.dket, self.dbra = dev(self.env), dev(self.w), dev(self.ket), dev(self.bra)
        self.dbra_c = dev(self.bra.conj())
        dd = self.dims = E.mpse_dims()
        dd.Dl_bra, dd.Dl_ket, dd.Dr_bra, dd.Dr_ket = Dlb, Dl, Drb, Dr
        dd.d0, dd.d1, dd.danc, dd.wl, dd.wm, dd.wr = d, 1, anc, wl, 1, wr
        self.oshape = (Drb, wr, Dr) if dom == "L" else (Dlb, wl, Dl)
        self.dtype = self.ket.dtype
        # the slice of one channel of the product env . ket
        self.macs = Db * Dk * d * anc * (Dr if dom == "L" else Dl)
        self.flops = self.macs * _flops_per_mac(self.denv.code, self.dket.code)

    def variants(self):
        """(name, bra tensor of the reference, bra_conj of the reference, device bra, bra_conj flag)"""
        v = [("bra", self.bra, True, self.dbra, 1), ("bra_preconj", self.bra.conj(), False, self.dbra_c, 0)]
        return v if self.separate_only else [("self", None, True, None, 1)] + v

    def run(self, unit, dbra, bra_conj, evidence=True):
        eng = self.eng
        self.dims.env_unit = unit
        out = eng.empty(self.oshape, self.dtype)

        def call():
            eng._check(eng.lib.mpse_env_update(eng.ctx, out.code, 0 if self.dom == "L" else 1, C.byref(self.dims),
                                               self.denv.ptr, self.denv.code, self.dket.ptr,
                                               None if dbra is None else dbra.ptr, bra_conj, self.dw.ptr, self.dw.code,
                                               out.ptr))
        if not evidence:
            call()
            return out.to_host(), None
        with Evidence(eng) as ev:
            call()
        return out.to_host(), ev


def _check_env_case(case, name, expect_shortcut=True):
    assert case.macs >= THRESHOLD, (name, case.macs)
    for vname, bra, conj, dbra, flag in case.variants():
        ref = cr.ref_env(case.dom, case.env, case.ket, case.w, bra=bra, bra_conj=conj)
        plain, ev0 = case.run(0, dbra, flag)
        out, ev = case.run(case.u + 1, dbra, flag)
        again, _ = case.run(case.u + 1, dbra, flag, evidence=False)
        dl, df = ev.paths["launches"] - ev0.paths["launches"], ev0.flops - ev.flops
        print(f"{name} {vname}: err {relerr(out, ref):.2e} plain {relerr(plain, ref):.2e} vs plain "
              f"{relerr(out, plain):.2e} launches {ev0.paths['launches']} {dl:+d} general {ev.paths['general']} "
              f"flops saved {df:.6g}")
        assert relerr(plain, ref) < 1e-12 and relerr(out, ref) < 1e-12, (name, vname)
        assert relerr(out, plain) < 1e-13, (name, vname)
        assert np.array_equal(out, again), (name, vname)
        assert ev.timed == ev.paths["launches"] and ev0.timed == ev0.paths["launches"]
        want_dl = _launch_delta(case.we, case.u) if expect_shortcut else 0
        want_df = case.flops if expect_shortcut else 0
        assert dl == want_dl, f"{name} {vname}: {dl:+d} launches against the plain plan, expected {want_dl:+d}"
        assert df == want_df, f"{name} {vname}: {df} flops saved, expected {want_df}"


ENV_SHAPES = {"site320": (320, (5,), 320, (3, 4)), "mpdm208": (208, (4, 4), 208, (4, 3))}


@pytest.mark.parametrize("pos", ["first", "mid", "last"])
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("dom", ["L", "R"])
@pytest.mark.parametrize("shape", list(ENV_SHAPES))
def test_env_update_unit_channel(eng, shape, dom, kind, pos):
    """both domains; bra = NULL, a separate bra conjugated by the call and one that is conjugated already"""
    Dl, phys, Dr, wb = ENV_SHAPES[shape]
    case = EnvCase(eng, dom, Dl, phys, Dr, wb, kind, pos, seed=_seed(shape, dom, kind, pos))
    _check_env_case(case, f"{shape}/{dom}/{kind}/{pos}")


@pytest.mark.parametrize("kind", ["f64", "c128"])
@pytest.mark.parametrize("dom", ["L", "R"])
def test_env_update_other_bra_bonds_ignore_the_unit(eng, dom, kind):
    """a bra with other bonds: the environment is rectangular and env_unit must be ignored"""
    case = EnvCase(eng, dom, 340, (5,), 340, (3, 4), kind, "mid", seed=23, bra_bonds=(300, 300))
    _check_env_case(case, f"rect300x340/{dom}/{kind}", expect_shortcut=False)
