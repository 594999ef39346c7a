"""The products with R of the folded one-site matvec inside a Krylov solve that holds the structural mask of its centre:
result tiles wholly outside the mask are not computed (MatvecReq::OutMask, mpse_gemm.hip `dead`) - nothing reads them.
Operands as in test_wfold_epilogue_gpu.py, the hop carrying ``centre_tile_mask`` of the same sector lists.  Every case is
solved here and, with MPSE_OUT_MASK=0, in ONE child process (the switch is read once per process): the results must be
bitwise equal - also where the masked launch runs its halved tiles in the eight-wave form (complex L: every halved case
here), whose dot partials are summed in the four-wave order (GemmGroups::dot4).  pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = -1e-7j

# name -> (Dl, d, Dr, cut of the two bond sectors (None: one sector), the skip is taken)
CASES = {
    "d16_cut100": (256, 16, 256, 100, True),      # sectors not tile aligned
    "d16_cut128": (256, 16, 256, 128, True),      # aligned
    "d8": (256, 8, 512, 100, True),               # 8 values of a per result tile
    "d32": (128, 32, 512, 100, True),             # 2 values of a per tile; more tiles than compute units: no halved tiles
    "d12": (320, 12, 256, 100, True),             # 64 % d != 0: a tile starts and ends inside a run of sigma
    "d16_one": (256, 16, 256, None, True),        # a single sector: every tile is live
}


def _band(rng, d, offsets):
    m = np.zeros((d, d))
    for o in offsets:
        m += np.diag(rng.uniform(0.5, 1.5, d - abs(o)) * rng.choice([-1.0, 1.0], d - abs(o)), o)
    return m


def _operands(name):
    """test_wfold_epilogue_gpu._operands with the cut of the sectors as a parameter; also the sector lists"""
    Dl, d, Dr, cut, _ = CASES[name]
    rng = np.random.default_rng(41)

    def rand(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    c0 = Dl if cut is None else cut
    c1 = Dr if cut is None else cut
    secl = np.array([0] * c0 + [1] * (Dl - c0))
    secr = np.array([0] * c1 + [1] * (Dr - c1))
    dq = np.array([0, 1, -1, 0, 0])
    l = rand((Dl, 5, Dl)) * (secl[:, None, None] - secl[None, None, :] == dq[None, :, None])
    r = rand((Dr, 4, Dr)) * (secr[:, None, None] - secr[None, None, :] == dq[None, :4, None])
    c = rand((Dl, d, Dr)) * (secl[:, None, None] == secr[None, None, :])
    l[:, 0, :] = np.eye(Dl)
    r[:, 3, :] = np.eye(Dr)
    w = np.zeros((5, d, d, 4))
    eye = np.eye(d)
    w[0, :, :, 0] = eye
    w[1, :, :, 1] = eye
    w[2, :, :, 2] = eye
    w[0, :, :, 3] = _band(rng, d, (-2, 0, 2))
    w[3, :, :, 3] = _band(rng, d, (-1, 0, 1))
    w[4, :, :, 3] = eye
    return l, r, w, c, secl, secr


def _hop(eng, name, masked=True, ru=True):
    from renormalizer_amd.mps.hop_expr import centre_tile_mask, hop_expr
    l, r, w, c, secl, secr = _operands(name)
    ld, rd = eng.asdevice(l), eng.asdevice(r)
    ld.unit, rd.unit = 1, (4 if ru else 0)
    hop = hop_expr(ld, rd, [w], c.shape)
    if masked:
        d = c.shape[1]
        hop.cmask = centre_tile_mask(eng, np.repeat(secl, d).reshape(-1, 1), -secr.reshape(-1, 1), np.zeros(1, dtype=int),
                                     c.shape)
        assert hop.cmask is not None
    return hop, c


def _stats(eng):
    return {**eng.gemm_path_stats(), **eng.wfold_path_stats()}


def _delta(a, b):
    return {k: b[k] - a[k] for k in b if b[k] != a[k]}


def solve(eng, name, masked=True):
    """(result, Krylov dimension, path counters of the solve, K tiles the c128 x c128 launches of the solve visited)"""
    from renormalizer_amd.lib.krylov import expm_krylov
    hop, c = _hop(eng, name, masked)
    v0 = eng.asdevice(c)
    eng.prof_enable(1)
    try:
        eng.prof_reset()
        s0 = _stats(eng)
        got, nvec = expm_krylov(hop, DT, v0)
        out = got.to_host()
        paths = _delta(s0, _stats(eng))
        ktiles = eng.prof_get()["c128xc128"]["ktiles"]
    finally:
        eng.prof_enable(0)
    return out, nvec, paths, ktiles


def ktile_counts(name):
    """K tiles of one matvec from the operands' non-zero patterns: (products with L, products with R over every result
    tile, products with R over the tiles the centre mask keeps)."""
    l, r, w, c, secl, secr = _operands(name)
    Dl, d, Dr = c.shape

    def occ(m):         # 64 x 16 tiles of a (rows, K) matrix that hold something
        return (np.abs(m) != 0).reshape(m.shape[0] // 64, 64, m.shape[1] // 16, 16).any(axis=(1, 3))
    allowed = np.broadcast_to(secl[:, None, None] == secr[None, None, :], c.shape).reshape(Dl, d * Dr)
    cm = allowed.reshape(Dl // 16, 16, d * Dr // 64, 64).any(axis=(1, 3))          # centre mask [a / 16, column / 64]
    # A: groups = the channels of L but its unit channel; K tiles with data in L's tile row and in the centre's tile column
    a_cnt = 0
    for b in range(1, 5):
        a_cnt += int((occ(l[:, b, :]).astype(int) @ cm.astype(int)).sum())
    # C: segments = the channels of R but its unit channel; the planes carry no mask, R's tile row decides
    per_tn = sum(occ(r[:, f, :]).sum(axis=1) for f in range(3))                   # [tn]
    tiles_m = Dl * d // 64
    live = np.zeros((tiles_m, Dr // 64), dtype=bool)
    for tm in range(tiles_m):
        for row in range(64 * tm, 64 * tm + 64):
            a, sg = divmod(row, d)
            for tn in range(Dr // 64):
                live[tm, tn] |= cm[a // 16, (sg * Dr + 64 * tn) // 64]
    return a_cnt, int(tiles_m * per_tn.sum()), int((live * per_tn[None, :]).sum()), live


_CHILD = """
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import test_out_mask_gpu as t
from renormalizer_amd import engine as E
eng = E.get_engine()
res = {{}}
for name in {names!r}:
    out, nvec, paths, ktiles = t.solve(eng, name)
    res[name] = out
    res[name + ":meta"] = np.array([nvec, paths.get("grouped", 0), paths.get("grouped_outmask", 0), ktiles])
np.savez({dst!r}, **res)
print("child ok")
"""


def _child(tmp, tag, env_kv, names):
    env = dict(os.environ)
    env.update(env_kv)
    dst = str(tmp / (tag + ".npz"))
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), names=list(names), dst=dst)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(dst)


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd import engine as E
    return E.get_engine()


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    """every case solved with MPSE_OUT_MASK=0, in one child process"""
    return _child(tmp_path_factory.mktemp("out_mask"), "off", {"MPSE_OUT_MASK": "0"}, CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_out_mask_solve(eng, switched_off, name):
    Dl, d, Dr, cut, taken = CASES[name]
    assert os.environ.get("MPSE_OUT_MASK", "1") != "0" and os.environ.get("MPSE_VEC_MASK", "1") != "0"
    out, nvec, paths, ktiles = solve(eng, name)
    ref = switched_off[name]
    nvec0, grouped0, om0, ktiles0 = (int(x) for x in switched_off[name + ":meta"])
    csteps = paths["grouped"] // 2
    a_cnt, c_all, c_live, live = ktile_counts(name)
    print(f"{name}: dim {nvec} / {nvec0}  paths {paths}  ktiles {ktiles} / {ktiles0}  per matvec A {a_cnt} C {c_all} "
          f"live {c_live}  live tiles {int(live.sum())} of {live.size}")
    # bitwise the solve that writes every tile
    assert nvec == nvec0
    assert np.array_equal(out, ref)
    # (how many matvecs a solve enqueues ahead of its decision depends on the context's earlier solves, the executed
    # ones do not: see the K tiles below)
    assert om0 == 0 and grouped0 >= 2
    # the plain solve: the identity channel of R not declared, no masks
    plain, n_plain = _plain(eng, name)
    assert n_plain == nvec
    err = float(np.abs(out - plain).max() / np.abs(plain).max())
    print(f"{name}: against the plain solve {err:.3e}")
    assert err < 1e-12, err
    # exact zeros outside the structural pattern
    _, _, _, c, secl, secr = _operands(name)
    allowed = np.broadcast_to(secl[:, None, None] == secr[None, None, :], c.shape)
    assert np.all(out[~allowed] == 0.0)
    # every launch that completes a result took the skip
    assert paths.get("grouped_outmask", 0) == (csteps if taken else 0), paths
    assert paths.get("grouped_split2", 0) == (0 if name == "d32" else csteps), paths
    # visited K tiles: whole matvecs of the solve, the products with R over the live tiles only
    per_on, per_off = a_cnt + (c_live if taken else c_all), a_cnt + c_all
    assert ktiles0 % per_off == 0 and ktiles % per_on == 0
    m = ktiles0 // per_off
    assert ktiles == m * per_on and nvec - 1 <= m <= csteps, (ktiles, ktiles0, m, csteps)
    if cut is None:
        assert live.all() and ktiles == ktiles0
    else:
        assert not live.all() and ktiles < ktiles0


def _plain(eng, name):
    from renormalizer_amd.lib.krylov import expm_krylov
    hop, c = _hop(eng, name, masked=False, ru=False)
    got, n = expm_krylov(hop, DT, eng.asdevice(c))
    return got.to_host(), n


def test_out_mask_not_taken(eng, tmp_path):
    """without the centre mask, for a plain product and with the vector kernels' mask off nothing is skipped"""
    name = "d16_cut100"
    _, _, paths, _ = solve(eng, name, masked=False)
    assert paths["grouped"] >= 2 and paths.get("grouped_outmask", 0) == 0, paths
    hop, c = _hop(eng, name)
    s0 = _stats(eng)
    hop(eng.asdevice(c))
    paths = _delta(s0, _stats(eng))
    assert paths["grouped"] == 2 and paths.get("grouped_outmask", 0) == 0, paths
    off = _child(tmp_path, "vec_mask_off", {"MPSE_VEC_MASK": "0"}, [name])
    nvec, grouped, om, _ = (int(x) for x in off[name + ":meta"])
    assert grouped >= 2 and om == 0
