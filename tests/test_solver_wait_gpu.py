"""The wait path of the device-decided solvers (publish_target / publish_collect, mpse_core.hip) without a mapped view of
the pinned mirror: a fresh process with MPSE_PINNED_MAP=0 - every read-back of a control block is then a copy - runs one
solve per driver (mpse_expm_lanczos, mpse_expm_lanczos_batch, mpse_pcg, mpse_pcg_batch), this process runs the same four
with the mapped view, and the results are compared bitwise: both solvers fix their answer on the device at the deciding
iteration, whenever and however the host looks."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
for _p in (TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

LZ_SHAPE = (32, 2, 32, 4)     # n = 2048 > 256: the asynchronous solve, small-centre matvec (d2D32 of test_batch_gpu.py)
PCG_DIMS, PCG_W = (8, 2, 8), 3


def run_solves():
    """{name: array} of one solve per driver: results, Krylov dimensions / iterations, statuses, batched members"""
    from renormalizer_amd import engine as E
    import test_batch_gpu as tb
    import test_pcg_batch_gpu as tp

    eng = E.get_engine()
    out = {}
    rng = np.random.default_rng(23)
    dt = complex(-0.4j)
    mem = [tb._member(eng, rng, LZ_SHAPE, True, scale=1.0 + 6.0 * k) for k in range(3)]
    st, x, nv = tb._single(eng, mem[0][0], mem[0][1], dt)
    out["lz_x"], out["lz_meta"] = x, np.array([st, nv])
    b0, s0 = tb._stats(eng)
    st, xs, nvs = tb._batch(eng, [m[0] for m in mem], [m[1] for m in mem], dt)
    b1, s1 = tb._stats(eng)
    out["lzb_x"], out["lzb_meta"] = np.stack(xs), np.array([st] + list(nvs))
    out["lzb_members"] = np.array([b1 - b0, s1 - s0])

    members = [tp.Member(eng, 100 + 7 * i, PCG_DIMS, PCG_W, True, True, domega=0.01 + 0.13 * i, shift=0.25 + 0.2 * i)
               for i in range(3)]
    m0 = members[0]
    db, dx, dd = m0.device()
    res = eng.pcg(m0.p.hop, db, dx, diag=dd, mask=m0.p.dmask, shift=m0.p.shift, tol=tp.TOL)
    out["pcg_x"], out["pcg_meta"] = dx.to_host(), np.array(tuple(res))
    res, xs, st = tp.solve(eng, members)
    out["pcgb_x"], out["pcgb_meta"] = np.stack(xs), np.array([tuple(r) for r in res])
    out["pcgb_members"] = np.array([st["batched_members"], st["single_members"]])
    return out


def test_copy_path_returns_the_same_bits():
    here = run_solves()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "copy_path.npz")
        env = dict(os.environ, MPSE_PINNED_MAP="0")
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, timeout=120,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert proc.returncode == 0, proc.stdout[-2000:]
        with np.load(path) as f:
            there = {k: f[k] for k in f.files}
    # the batched kernels ran in both processes: three members each, none through the single solve
    for got in (here, there):
        assert list(got["lzb_members"]) == [3, 0] and list(got["pcgb_members"]) == [3, 0]
    assert here["lz_meta"][0] == 0 and here["lzb_meta"][0] == 0
    assert not here["pcg_meta"][0] and not here["pcgb_meta"][:, 0].any()
    assert sorted(here) == sorted(there)
    for k in here:     # x / out, Krylov dimension or iterations, status, relres, lvalue
        assert here[k].dtype == there[k].dtype and np.array_equal(here[k], there[k]), k


if __name__ == "__main__":
    assert os.environ.get("MPSE_PINNED_MAP") == "0"
    np.savez(sys.argv[1], **run_solves())
