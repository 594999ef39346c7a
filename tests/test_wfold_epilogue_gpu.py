"""The folded one-site matvec with the plane of R's unit channel formed in the epilogue of the first product with R
(mpse_plans.h EpiTerm, mpse_gemm.hip `mix_on`) against the oracle, at the smallest centres that take the folded plan
without a hook (Dl d Dr Dl >= 2^28); the sites that do not qualify keep the elementwise pass (k_wmix).  The switches are
read once per process, so MPSE_WFOLD_EPI=0 and MPSE_SPLIT2=0 run the same cases in a child process.  pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (Dl, d, Dr, kind of the plane of R's unit channel, R's unit channel declared, forms the plane in the epilogue)
CASES = {
    "d16": (256, 16, 256, "band", True, True),
    "d8": (256, 8, 512, "band", True, True),
    "d32": (128, 32, 512, "band", True, True),
    "dense": (256, 16, 256, "dense", True, False),      # a dense block in the plane
    "no_ru": (256, 16, 256, "band", False, False),      # the identity channel of R not declared: no plane is `out`
    "d12": (320, 12, 256, "band", True, False),         # 64 % 12 != 0
}


def _band(rng, d, offsets):
    m = np.zeros((d, d))
    for o in offsets:
        m += np.diag(rng.uniform(0.5, 1.5, d - abs(o)) * rng.choice([-1.0, 1.0], d - abs(o)), o)   # first and last rows too
    return m


def _operands(name):
    """Block-sparse operands with two bond sectors that do not align with the 64-wide tiles, and a (5, d, d, 4) site
    whose plane of R's unit channel (3) is an identity block + a band(+-2) block on the centre + a tridiagonal block."""
    Dl, d, Dr, kind, ru_known, _ = CASES[name]
    rng = np.random.default_rng(41)

    def rand(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    secl = np.array([0] * 100 + [1] * (Dl - 100))
    secr = np.array([0] * 100 + [1] * (Dr - 100))
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
    w[3, :, :, 3] = _band(rng, d, (-1, 0, 1)) if kind == "band" else rng.standard_normal((d, d))
    w[4, :, :, 3] = eye
    return l, r, w, c, (4 if ru_known else 0)


def _relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(b).max()))


def _hop(eng, name):
    from renormalizer_amd.mps.hop_expr import hop_expr
    l, r, w, c, ru = _operands(name)
    ld, rd = eng.asdevice(l), eng.asdevice(r)
    ld.unit, rd.unit = 1, ru
    return hop_expr(ld, rd, [w], c.shape), c


def _stats(eng):
    return {**eng.gemm_path_stats(), **eng.wfold_path_stats()}


def _delta(a, b):
    return {k: b[k] - a[k] for k in b if b[k] != a[k]}


def check_case(eng, name, ref, epi_on=True, split2_on=True):
    """one product against the oracle's result, which launches it took, a zero centre, and the product inside a
    Krylov solve (halved tiles, the dot partials riding on the last launch) against the plain solve"""
    from renormalizer_amd.lib.krylov import expm_krylov
    mixes = CASES[name][5] and epi_on
    hop, c = _hop(eng, name)
    s0 = _stats(eng)
    out = hop(eng.asdevice(c)).to_host()
    paths = _delta(s0, _stats(eng))
    err = _relerr(out.ravel(), ref.ravel())
    print(f"{name}: epi={epi_on} split2={split2_on} relerr {err:.3e} paths {paths}")
    assert err < 1e-12, (name, err)
    assert paths.get("grouped") == 2, paths
    assert paths.get("grouped_mix", 0) == (1 if mixes else 0), paths
    assert paths.get("wmix", 0) == (0 if mixes else 1), paths
    z = hop(eng.zeros(c.shape, c.dtype)).to_host()
    assert np.abs(z).max() == 0.0
    if name != "d16":
        return
    # The solve takes the result in two parts (halved tiles unless MPSE_SPLIT2=0) and its first Lanczos coefficient from
    # the dot partials of the launch that carries the mix.  The plain solve: the same operator with the identity
    # channel of R not declared - every plane through the elementwise pass, all products with R.  With a tiny step
    # both stop at their second estimate.
    v0 = eng.asdevice(c)
    s0 = _stats(eng)
    got, n1 = expm_krylov(hop, -1e-7j, v0)
    paths = _delta(s0, _stats(eng))
    assert paths.get("grouped_mix", 0) == (paths["grouped"] // 2 if mixes else 0), paths
    assert paths.get("wmix", 0) == (0 if mixes else paths["grouped"] // 2), paths
    assert (paths.get("grouped_split2", 0) > 0) == split2_on, paths
    plain_hop, _ = _hop(eng, "no_ru")
    plain, n0 = expm_krylov(plain_hop, -1e-7j, v0)
    err = _relerr(got.to_host().ravel(), plain.to_host().ravel())
    print(f"{name}: krylov dims {n1} / {n0} relerr {err:.3e}")
    assert n0 == n1
    assert err < 1e-12, err


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd import engine as E
    return E.get_engine()


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """the oracle's results, computed once: the child processes read them from the file"""
    from oracle import mps_oracle as orc
    from conftest import oracle_threads
    out = {}
    with oracle_threads():
        for name in CASES:
            l, r, w, c, _ = _operands(name)
            out[name] = orc.hop_apply(l, r, [w], c)
    path = str(tmp_path_factory.mktemp("wfold_epi") / "refs.npz")
    np.savez(path, **out)
    return out, path


@pytest.mark.parametrize("name", list(CASES))
def test_epilogue_mix_vs_oracle(eng, refs, name):
    check_case(eng, name, refs[0][name], epi_on=os.environ.get("MPSE_WFOLD_EPI", "1") != "0",
               split2_on=os.environ.get("MPSE_SPLIT2", "1") != "0")


_CHILD = """
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import test_wfold_epilogue_gpu as t
from renormalizer_amd import engine as E
eng = E.get_engine()
refs = np.load({refs!r})
for name in t.CASES:
    t.check_case(eng, name, refs[name], epi_on={epi}, split2_on={split2})
print("child ok")
"""


@pytest.mark.parametrize("switch", ["MPSE_WFOLD_EPI=0", "MPSE_SPLIT2=0"])
def test_epilogue_mix_switches(refs, switch):
    """the same cases with the epilogue mix off (the elementwise pass everywhere) and with one workgroup per tile"""
    env = dict(os.environ)
    k, v = switch.split("=")
    env[k] = v
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), refs=refs[1],
                         epi=(switch != "MPSE_WFOLD_EPI=0") and os.environ.get("MPSE_WFOLD_EPI", "1") != "0",
                         split2=(switch != "MPSE_SPLIT2=0") and os.environ.get("MPSE_SPLIT2", "1") != "0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
