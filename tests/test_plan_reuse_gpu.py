"""Plan re-use across solves (mpse_solve_slot, mpse_ctx::plan_store): a keyed solve is bitwise its keyless self, whatever
its slot holds, and the device rebuilds a kept plan exactly when a flag byte it was built from differs.

The operands are those of the fused bond / two-level-site matvec (mpse_heff0.hip) at the smallest bond at which the solve
takes it by default (192: twelve tiles a side, three 64-column chunks; centres of up to 32 768 elements go to the
one-launch matvec of small centres): block-sparse Hermitian environments of two quantum-number
sectors cut at ``cut``, a centre inside the sectors, optionally with its structural mask.  The reference of every
case is the solve of the same operands without a key.
"""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.mps.hop_expr import centre_tile_mask, hop_expr

from kron_problems import _rand   # (tests/kron_problems.py)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the counters move only where keys are honoured and the fused matvec runs (the asynchronous solve drives it); the
# bitwise property holds under every switch and is asserted always
FUSED = os.environ.get("MPSE_HEFF0", "1") != "0" and os.environ.get("MPSE_LANCZOS_ASYNC", "1") != "0"
ON = os.environ.get("MPSE_PLAN_REUSE", "1") != "0" and FUSED
DT = -0.3j


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def _sectors(D, cut):
    return (np.arange(D) >= cut).astype(int)


def _herm(rng, n, sec):
    x = _rand(rng, (n, n), True) * (sec[:, None] == sec[None, :]) / (4 * np.sqrt(n))
    return x + x.conj().T


def _bond(seed, Dl, Dr, cut, w=3):
    """bond problem: (l, r, c, sl, sr); every channel keeps the sector, channel 0 / w - 1 carry the identities"""
    rng = np.random.default_rng(seed)
    sl, sr = _sectors(Dl, cut), _sectors(Dr, cut)
    l = np.stack([np.eye(Dl) if b == 0 else _herm(rng, Dl, sl) for b in range(w)], axis=1)
    r = np.stack([np.eye(Dr) if b == w - 1 else _herm(rng, Dr, sr) for b in range(w)], axis=1)
    c = _rand(rng, (Dl, Dr), True) * (sl[:, None] == sr[None, :])
    return l, r, c, sl, sr


OPS = [np.eye(2), np.array([[0.0, 1.0], [1.0, 0.0]]), np.diag([0.0, 1.0]), np.array([[0.3, -0.7], [-0.7, 0.1]])]


def _site_w(w, other=False):
    wm = np.zeros((w, 2, 2, w))
    for b in range(w):
        wm[b, :, :, b] = OPS[(b + (2 if other else 0)) % 4]
    return wm


def _site(seed, D, cut, w=3, other_w=False):
    """two-level-site problem: (l, r, wm, c, sl, sr)"""
    rng = np.random.default_rng(seed)
    sl, sr = _sectors(D, cut), _sectors(D, cut)
    l = np.stack([np.eye(D) if b == 0 else _herm(rng, D, sl) for b in range(w)], axis=1)
    r = np.stack([np.eye(D) if b == w - 1 else _herm(rng, D, sr) for b in range(w)], axis=1)
    c = _rand(rng, (D, 2, D), True) * (sl[:, None, None] == sr[None, None, :])
    return l, r, _site_w(w, other_w), c, sl, sr


def _solve(eng, hop, c, key=0, cmask=None):
    """(result on the host, nvec) of mpse_expm_lanczos under `key`"""
    cd = eng.asdevice(c)
    out = eng.empty(cd.shape, cd.dtype)
    nv = C.c_int()
    if cmask is not None:
        eng._check(eng.lib.mpse_expm_centre_mask(eng.ctx, cmask.ptr, cmask.nbytes))
    if key:
        eng._check(eng.lib.mpse_solve_slot(eng.ctx, key))
    eng._check(eng.lib.mpse_expm_lanczos(eng.ctx, cd.code, C.byref(hop.heff), DT.real, DT.imag, cd.ptr, out.ptr, 1e-10,
                                         0.0, 0, C.byref(nv)))
    return out.to_host(), nv.value


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _keyed(eng, hop, c, key, cmask=None):
    """keyed solve: (result, nvec, counter deltas, fused launches)"""
    s0, f0 = eng.plan_reuse_stats(), sum(eng.heff_fused_stats())
    out, nv = _solve(eng, hop, c, key, cmask)
    return out, nv, _delta(s0, eng.plan_reuse_stats()), sum(eng.heff_fused_stats()) - f0


def _check(eng, hop, c, key, want, cmask=None, **counts):
    """a keyed solve equals the keyless `want` = (result, nvec) bitwise, ran fused, and moved the counters by `counts`"""
    out, nv, d, fused = _keyed(eng, hop, c, key, cmask)
    assert nv == want[1] and np.array_equal(out, want[0])
    if FUSED:
        assert fused >= nv                       # the matvecs of the solve went through the fused launch
    if ON:
        assert d["keyed"] == 1
        for k, v in counts.items():
            assert d[k] == v, (k, d)
    else:
        assert not any(d[k] for k in ("hits", "mismatches", "evictions", "fused_rebuilds")), d
    return d


def test_same_key_other_structure(eng):
    """A, B of equal shapes with another sector cut, A again under one key: each bitwise keyless, the plan rebuilt on
    every change of structure and kept when the structure repeats"""
    key = 1001
    for make in (lambda cut: _bond(5, 192, 192, cut), lambda cut: _site(6, 192, cut)):
        pa, pb = make(96), make(128)
        hops = [hop_expr(p[0], p[1], list(p[2:-3]), p[-3].shape) for p in (pa, pb)]
        want = [_solve(eng, h, p[-3]) for h, p in zip(hops, (pa, pb))]
        assert not np.array_equal(want[0][0], want[1][0])
        _check(eng, hops[0], pa[-3], key, want[0], fused_rebuilds=1)                  # fresh slot (or another shape)
        _check(eng, hops[0], pa[-3], key, want[0], hits=1, fused_rebuilds=0)          # kept
        _check(eng, hops[1], pb[-3], key, want[1], hits=1, fused_rebuilds=1)          # A -> B
        _check(eng, hops[1], pb[-3], key, want[1], hits=1, fused_rebuilds=0)
        _check(eng, hops[0], pa[-3], key, want[0], hits=1, fused_rebuilds=1)          # B -> A
        key += 1


@pytest.mark.parametrize("which", ["L", "R", "mask"])
def test_one_tile(eng, which):
    """one 16 x 16 tile of L / of R emptied, one byte of the centre mask raised, between two keyed solves: a rebuild
    and the keyless result on the modified operands; put back: another rebuild and the first result (both directions,
    occupied -> empty and empty -> occupied)"""
    key = {"L": 2001, "R": 2002, "mask": 2003}[which]
    l, r, c, sl, sr = _bond(11, 192, 192, 96)
    cmask = centre_tile_mask(eng, sl[:, None], (1 - sr)[:, None], np.array([1]), c.shape)
    assert cmask is not None
    l2, r2, cmask2 = l.copy(), r.copy(), cmask
    if which == "L":
        assert np.any(l2[16:32, 1, 16:32] != 0)
        l2[16:32, 1, 16:32] = 0                      # (a diagonal tile: the operator stays Hermitian)
    elif which == "R":
        assert np.any(r2[80:96, 0, 80:96] != 0)
        r2[80:96, 0, 80:96] = 0
    else:
        m = cmask.to_host().copy()
        flat = m.reshape(-1).view(np.uint8)
        # the first tile the mask leaves out (inside the 12 tile bytes of a row): a superset mask, same mathematics
        nkt = 192 // 16
        rows = flat.reshape(-1, 8 * ((nkt + 7) // 8))[:, :nkt]
        i, j = np.argwhere(rows == 0)[0]
        rows[i, j] = 1
        cmask2 = eng.asdevice(m)
        assert cmask2.nbytes == cmask.nbytes
    hop, hop2 = hop_expr(l, r, [], c.shape), hop_expr(l2, r2, [], c.shape)
    want, want2 = _solve(eng, hop, c, cmask=cmask), _solve(eng, hop2, c, cmask=cmask2)
    _check(eng, hop, c, key, want, cmask, fused_rebuilds=1)
    _check(eng, hop, c, key, want, cmask, hits=1, fused_rebuilds=0)
    _check(eng, hop2, c, key, want2, cmask2, hits=1, fused_rebuilds=1)
    _check(eng, hop2, c, key, want2, cmask2, hits=1, fused_rebuilds=0)
    _check(eng, hop, c, key, want, cmask, hits=1, fused_rebuilds=1)
    _check(eng, hop, c, key, want, cmask, hits=1, fused_rebuilds=0)


def test_host_side_mismatch(eng):
    """one key, then another shape, then another MPO site of the same shape: keyless results, counted mismatches"""
    key = 3001
    l, r, wm, c, _, _ = _site(21, 192, 96)
    hop = hop_expr(l, r, [wm], c.shape)
    _check(eng, hop, c, key, _solve(eng, hop, c), fused_rebuilds=1)
    # another shape (a bond matrix with another right bond)
    lb, rb, cb, _, _ = _bond(22, 192, 256, 96)
    hopb = hop_expr(lb, rb, [], cb.shape)
    _check(eng, hopb, cb, key, _solve(eng, hopb, cb), hits=0, mismatches=1, fused_rebuilds=1)
    _check(eng, hop, c, key, _solve(eng, hop, c), hits=0, mismatches=1, fused_rebuilds=1)
    # another MPO site between the same environments: same shapes, another term table
    wm2 = _site_w(3, True)
    assert not np.array_equal(wm2, wm)
    hop2 = hop_expr(l, r, [wm2], c.shape)
    want2 = _solve(eng, hop2, c)
    _check(eng, hop2, c, key, want2, hits=0, mismatches=1, fused_rebuilds=1)
    _check(eng, hop2, c, key, want2, hits=1, mismatches=0, fused_rebuilds=0)


def test_eviction(eng):
    """a budget that holds one slot, three keys in turn: slots go, every result stays keyless, and the pool's bytes in
    use do not grow from one round to the next"""
    l, r, c, _, _ = _bond(31, 192, 192, 96)
    hop = hop_expr(l, r, [], c.shape)
    want = _solve(eng, hop, c)
    eng._check(eng.lib.mpse_plan_store_budget(eng.ctx, 20000))          # (one slot of this problem: about 12 kB)
    try:
        used = []
        for rnd in range(3):
            ev = 0
            for key in (4001, 4002, 4003):
                d = _check(eng, hop, c, key, want, hits=0, fused_rebuilds=1)
                ev += d["evictions"]
            # (the first round also clears what earlier tests left; from then on every key finds its slot gone)
            if ON:
                assert ev >= 2 if rnd == 0 else ev == 3, (rnd, ev)
            gc.collect()
            used.append(eng.mem_info()["in_use"])
        assert used[1] == used[2], used
    finally:
        eng._check(eng.lib.mpse_plan_store_budget(eng.ctx, 64 << 20))
    _check(eng, hop, c, 4003, want, hits=1, fused_rebuilds=0)           # the last slot is still there


# ------------------------------------------------------------------------------------------- child processes

_EVOLVES = r"""
import sys, numpy as np
sys.path.insert(0, {repo!r})
from renormalizer_amd import HolsteinModel, Phonon, Mol, Quantity, Mpo, EvolveConfig, EvolveMethod
from renormalizer_amd.engine import get_engine
from renormalizer_amd.mps.mps import Mps
ph = Phonon.simple_phonon(Quantity(6.128e-3), Quantity(16.274571056529368), 16)
model = HolsteinModel([Mol(Quantity(0), [ph])] * 4, Quantity(3.0e-2), 3)
mpo = Mpo(model)
mps = Mps.random(model, 1, 64, rng=np.random.default_rng(7))
mps.evolve_config = EvolveConfig(EvolveMethod.tdvp_ps)
eng = get_engine()
stats, steps = [], []
for _ in range(3):
    mps = mps.evolve(mpo, 10.0)
    s = eng.plan_reuse_stats()
    stats.append([s[k] for k in eng.PLAN_REUSE])
    steps.append(list(mps.evolve_config.stat["steps"]))
np.savez({out!r}, stats=np.array(stats), steps=np.array(steps), dims=np.array(mps.bond_dims),
         fused=np.array(eng.heff_fused_stats()), **{{f"s{{i}}": a for i, a in enumerate(mps.to_arrays())}})
"""


def _evolves(tmp, tag, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = str(tmp / f"{tag}.npz")
    r = subprocess.run([sys.executable, "-c", _EVOLVES.format(repo=REPO, out=out)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def evolved(tmp_path_factory):
    """three evolves of a short Holstein chain (d = 2 / 16 alternating, interior bonds 64; MPSE_HEFF0=2, MPSE_SMALL=0: the
    fused matvec at every eligible size, the small centres through the plans) in fresh processes: default, MPSE_PLAN_REUSE=0, MPSE_F0_ORDER=0"""
    tmp = tmp_path_factory.mktemp("plan_reuse")
    base = {"MPSE_HEFF0": "2", "MPSE_SMALL": "0"}
    return {tag: _evolves(tmp, tag, {**base, **extra})
            for tag, extra in (("default", {}), ("off", {"MPSE_PLAN_REUSE": "0"}), ("plain", {"MPSE_F0_ORDER": "0"}))}


_DESTROY = r"""
import gc, json, sys, ctypes as C, numpy as np
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import test_plan_reuse_gpu as T
from renormalizer_amd.engine import get_engine
from renormalizer_amd.mps.hop_expr import hop_expr
eng = get_engine()
l, r, c, _, _ = T._bond(41, 192, 192, 96)
hop = hop_expr(l, r, [], c.shape)
want = T._solve(eng, hop, c)
T._solve(eng, hop, c, 5000)                                   # (the context's counter words exist from here on)
budget = lambda b: eng._check(eng.lib.mpse_plan_store_budget(eng.ctx, b))
def used():
    gc.collect()
    return eng.mem_info()["in_use"]
budget(0)
base, s0 = used(), eng.plan_reuse_stats()
budget(20000)
same, ev = True, []
for rnd in range(2):
    e0 = eng.plan_reuse_stats()["evictions"]
    for key in (5001, 5002, 5003):
        out, nv = T._solve(eng, hop, c, key)
        same = same and nv == want[1] and bool(np.array_equal(out, want[0]))
    ev.append(eng.plan_reuse_stats()["evictions"] - e0)
held = used() - base
budget(0)
freed = used() - base
budget(64 << 20)
out, nv = T._solve(eng, hop, c, 5001)                          # a live slot goes down with the context
same = same and bool(np.array_equal(out, want[0]))
live = used() - base
s1 = eng.plan_reuse_stats()
st = eng.lib.mpse_ctx_destroy(eng.ctx)
eng.ctx = None
print(json.dumps(dict(same=same, ev=ev, held=held, freed=freed, live=live, destroy=st,
                      evictions=s1["evictions"] - s0["evictions"], keyed=s1["keyed"] - s0["keyed"])))
"""


def test_eviction_accounting_and_destroy(tmp_path):
    """a context of its own (child process): keys cycled under a budget of one slot, then the budget taken to zero - the
    pool's bytes in use are back where they were before the first slot, every eviction is counted - and the context is
    destroyed while a slot is alive"""
    import json
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    code = _DESTROY.format(repo=REPO, tests=os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print(got)
    assert got["same"] and got["destroy"] == 0, got
    assert got["freed"] == 0, got                 # nothing of the slots is left in use once they are gone
    if ON:
        assert got["ev"] == [2, 3], got           # an empty store: the first key fits; later every key finds its slot gone
        assert 0 < got["held"] <= 20000 + 4096 and 0 < got["live"] <= 20000 + 4096, got     # one slot (pool bucket slack)
        assert got["evictions"] == 6 and got["keyed"] == 7, got                             # 2 + 3 + the trim to zero
    else:
        assert got["held"] == 0 and got["live"] == 0 and got["evictions"] == 0, got


def _same_state(a, b):
    assert np.array_equal(a["dims"], b["dims"]) and np.array_equal(a["steps"], b["steps"])
    for i in range(len(a["dims"]) - 1):
        assert np.array_equal(a[f"s{i}"], b[f"s{i}"]), i


def test_evolves_bitwise_and_kept(evolved):
    """default against MPSE_PLAN_REUSE=0: the same bits; the slots are hit from the second evolve on and the device
    rebuilds no plan in the third"""
    on, off = evolved["default"], evolved["off"]
    _same_state(on, off)
    assert np.array_equal(on["fused"], off["fused"])
    assert not off["stats"].any()
    if not ON:
        assert not on["stats"][:, 1:].any()
        return
    assert on["fused"].sum() > 0
    names = list(E.Engine.PLAN_REUSE)
    per = np.diff(np.vstack([np.zeros((1, len(names)), dtype=on["stats"].dtype), on["stats"]]), axis=0)
    print("plan re-use per evolve:", [dict(zip(names, row.tolist())) for row in per])
    ik, ih, ir = names.index("keyed"), names.index("hits"), names.index("fused_rebuilds")
    for e in (1, 2):
        assert per[e][ik] > 0 and per[e][ih] > 0, per
    assert per[2][ir] == 0, per


def test_keyed_plain_order(evolved):
    """keyed solves with MPSE_F0_ORDER=0 (k_f0_valid under the same rule): bitwise the default, nothing rebuilt in the
    third evolve"""
    _same_state(evolved["plain"], evolved["default"])
    st = evolved["plain"]["stats"]
    if not ON:
        return
    ir = list(E.Engine.PLAN_REUSE).index("fused_rebuilds")
    assert st[2][ir] == st[1][ir] and st[2][1] > st[1][1], st
