"""k_heff0_fused (csrc/mpse_heff0.hip) at every edge of its tiling and bookkeeping, through the only entry it has - the
Lanczos solve that consumes its tile-masked parts - against the oracle's float64 solve of the same problem.

The problems and what each is for are in tests/heff0_problems.py (CASES); test_heff0_problems_host.py holds each case to
the structure it is named for and measures the reference (rounding 3e-15 against the Krylov estimate of the same
dimension, so the 1e-10 asserted here is the bound of the existing fused tests and far above the reference's own error).
Every shape has both bonds >= 128 and is beyond the one-launch matvec of small centres, so the default mode takes (or
refuses) the fused launch in this process: no switch, no child.

Per case: three solves; the launch counter of the right kind moved by exactly 3 * nvec and the other not at all (refused
cases: neither); nvec is the oracle's; |out - ref| <= 1e-10 |ref|; the three results are bitwise equal; every element in an
output tile that the census says no unit holds, and everything outside the quantum-number blocks, is exactly 0.

Shapes that differ from the table of the issue that asked for these tests:
  * site_16_terms / site_17_terms run at 144 x 2 x 128, not 128 x 2 x 128: a centre of 32 768 elements with at most eight
    MPO channels belongs to the one-launch matvec of small centres (small_plan, csrc/mpse_small.hip), whatever the fused
    path would say.  (bond_64_parts keeps 128 x 256: sixteen channels are more than that kernel takes.)
  * bond_w_mismatch: a bond matrix between environments of three and four channels is not a contraction
    (abc,lbk,ck->al shares b); the engine refuses it with an error from the plans and launches nothing - asserted - and
    the same operands padded to four channels on both sides (one of zeros) are the case bond_w_padded of the table.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from renormalizer_amd import engine as E
from renormalizer_amd.lib.krylov import expm_krylov
from renormalizer_amd.mps.hop_expr import centre_tile_mask, hop_expr

import heff0_problems as P          # (tests/heff0_problems.py)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the counters move only where the fused matvec is on and the asynchronous solve drives it; everything else holds always
FUSED = os.environ.get("MPSE_HEFF0", "1") != "0" and os.environ.get("MPSE_LANCZOS_ASYNC", "1") != "0"
KIND = {"bond": 0, "site": 1}
_first = {}          # case id -> first result of this process (test_plain_order_bitwise compares a child's with it)


@pytest.fixture(scope="module")
def eng():
    return E.get_engine()


def _hop(eng, cid, p):
    hop = hop_expr(p.l, p.r, p.cmo, p.c.shape)
    if p.qn is not None:
        hop.cmask = centre_tile_mask(eng, *p.qn, p.c.shape)
        assert hop.cmask is not None
    if cid == "bond_mask_other_shape":
        # a mask for a 128 x 192 bond matrix on a 192 x 192 one: its size says so, and nothing may use it
        sl, sr = P.cut(128, 4), P.cut(192, 6)
        hop.cmask = centre_tile_mask(eng, sl[:, None], (1 - sr)[:, None], np.array([1]), (128, 192))
        assert hop.cmask is not None and hop.cmask.nbytes == 24          # (this shape's own has 48)
    return hop


def _solve(eng, cid):
    """(problem, three results on the host, their Krylov dimensions, movement of the (bond, site) launch counters)"""
    p = P.build(cid)
    hop = _hop(eng, cid, p)
    f0 = eng.heff_fused_stats()
    outs, nvs = [], []
    for _ in range(3):
        out, nv = expm_krylov(hop, p.dt, eng.asdevice(p.c))
        outs.append(out.to_host())
        nvs.append(nv)
    f1 = eng.heff_fused_stats()
    return p, outs, nvs, (f1[0] - f0[0], f1[1] - f0[1])


def _check(eng, cid):
    from conftest import oracle_threads
    p, outs, nvs, moved = _solve(eng, cid)
    _first[cid] = outs[0]
    with oracle_threads():
        ref, nref = p.reference()
    path = P.CASES[cid][0]
    err = np.linalg.norm(outs[0].ravel() - ref) / np.linalg.norm(ref)
    print(f"{cid}: nvec {nvs} (oracle {nref}), launches (bond, site) {moved}, |out - ref| / |ref| = {err:.2e}")
    if FUSED:
        want = [0, 0]
        if path is not None:
            want[KIND[path]] = 3 * nref
        assert list(moved) == want
    assert nvs == [nref] * 3
    assert err <= 1e-10
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    z = p.must_be_zero
    assert not outs[0][z].any()
    return p, outs[0]


@pytest.mark.parametrize("cid", list(P.CASES))
def test_fused_matvec_edges(eng, cid):
    _check(eng, cid)


def test_bond_w_mismatch_is_refused(eng):
    """three channels on the left, four on the right: an error, not a launch and not a silent result"""
    p = P.build("bond_w_padded")
    assert not p.l[:, 3, :].any()
    hop = hop_expr(np.ascontiguousarray(p.l[:, :3, :]), p.r, [], p.c.shape)
    assert (hop.heff.dims.wl, hop.heff.dims.wr) == (3, 4)
    f0 = eng.heff_fused_stats()
    with pytest.raises(ValueError, match="wl != wr"):
        expm_krylov(hop, p.dt, eng.asdevice(p.c))
    assert eng.heff_fused_stats() == f0
    _check(eng, "bond_w_padded")                    # the engine is none the worse for it, and the padded operator is served


_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import test_heff0_fused_gpu as T
from renormalizer_amd.engine import get_engine
eng = get_engine()
res = {{}}
for cid in T.P.CASES:
    p, outs, nvs, moved = T._solve(eng, cid)
    res["out_" + cid], res["nv_" + cid], res["moved_" + cid] = outs[0], np.array(nvs), np.array(moved)
np.savez({out!r}, **res)
"""


def test_plain_order_bitwise(eng, tmp_path):
    """MPSE_F0_ORDER=0 (read once per process, so ONE fresh process runs the whole table): units launched in index order
    with the part mask of k_f0_valid write the same tiles into the same slots - every result bitwise this process's."""
    for cid in P.CASES:
        if cid not in _first:
            _first[cid] = _solve(eng, cid)[1][0]
    env = dict(os.environ)
    env["MPSE_F0_ORDER"] = "0"
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = str(tmp_path / "plain.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), out=out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.load(out)
    for cid, (path, _, _, _) in P.CASES.items():
        nv, moved = got["nv_" + cid], got["moved_" + cid]
        assert nv[0] == nv[1] == nv[2]
        if FUSED:
            want = [0, 0]
            if path is not None:
                want[KIND[path]] = 3 * int(nv[0])
            assert moved.tolist() == want, cid
        assert np.array_equal(got["out_" + cid], _first[cid]), cid
