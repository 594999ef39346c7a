"""Seeded chains of site tensors and MPO sites, and the path assertion, shared by the GPU tests of the one-call chain
entry points (test_overlap_gpu.py, test_sandwich_gpu.py, test_corr_gpu.py).  Every array draws its real part and then,
when complex, its imaginary part from the generator it is given, site after site."""
import numpy as np


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def _flags(c, n):
    return [c] * n if isinstance(c, bool) else list(c)


def _chain(rng, bonds, ds, cplx, danc=None):
    """site tensors (bonds[i], ds[i].., [danc[i],] bonds[i + 1]); ds[i]: one extent or a tuple of them; cplx: one flag
    or one per site"""
    fl = _flags(cplx, len(ds))
    return [_rand(rng, (bonds[i],) + (tuple(d) if isinstance(d, tuple) else (d,)) + (() if danc is None else (danc[i],))
                  + (bonds[i + 1],), fl[i]) for i, d in enumerate(ds)]


def _mpo(rng, wb, ds, cplx):
    fl = _flags(cplx, len(ds))
    return [_rand(rng, (wb[i], d, d, wb[i + 1]), fl[i]) for i, d in enumerate(ds)]


def _dev(eng, arrays):
    return [eng.asdevice(np.ascontiguousarray(a)) for a in arrays]


def took_path(stats_fn, call, path, nsites):
    """call() between two readings of stats_fn(): asserts that it counted once on ``path`` ("chain_kernel" or
    "enqueued"), not on the other one, and walked ``nsites`` sites; returns (value of call(), stats before, after)"""
    s0 = stats_fn()
    got = call()
    s1 = stats_fn()
    other = "enqueued" if path == "chain_kernel" else "chain_kernel"
    assert s1[path] - s0[path] == 1 and s1[other] == s0[other] and s1["sites"] - s0["sites"] == nsites, (path, s0, s1)
    return got, s0, s1
