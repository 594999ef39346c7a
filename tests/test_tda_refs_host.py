"""The NumPy restatement of the tangent-space operator (tests/tda_refs.py) against dense matrices, without a GPU: it is
the reference of tests/test_tda_gpu.py, so its own error has to sit well inside the bound asserted there
(1e-12 |x|_2 prod_i |W_i|_F per entry).  Also: the new entry points are declared, bound and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tda_refs as tr                                  # (tests/tda_refs.py)
from renormalizer_amd import engine as E

NAMES = ("mpse_tda_create", "mpse_tda_destroy", "mpse_tda_apply", "mpse_tda_hdiag", "mpse_tda_davidson",
         "mpse_tda_stats")
ALL = [(c, k) for c in tr.CASES for k in tr.KINDS]


def _psi0(B):
    t = np.ones((1, 1))
    for b in B:
        t = np.tensordot(t, b, axes=(1, 0)).reshape(-1, b.shape[2])
    return t[:, 0]


def test_header_binding_and_library_agree():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "mpsengine.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(E.LIB_PATH)
    for name in NAMES:
        assert f"int {name}(" in header and name in E.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert E.Engine.TDA_STATS == ("handles", "applies", "env_updates", "heff_applies", "qdiag_sites", "davidson")
    from renormalizer_amd.mps import TDA                # exported from the mps package
    assert TDA.__module__ == "renormalizer_amd.mps.tda"


@pytest.mark.parametrize("case,kind", ALL)
def test_projector_is_an_isometry_orthogonal_to_the_state(case, kind):
    A, B, U, W = tr.problem(case, kind)
    P = tr.dense_p(A, B, U)
    n = P.shape[1]
    assert n == tr.xsize(B, U)
    assert np.abs(P.conj().T @ P - np.eye(n)).max() <= 1e-13
    psi = _psi0(B)
    assert abs(np.linalg.norm(psi) - 1.0) <= 1e-13
    ov = P.conj().T @ psi
    if tr.CASES[case][3]:                              # include_psi0: the state lies in the span of the last block
        nlast = U[-1].shape[2]
        assert np.abs(ov[:-nlast]).max() <= 1e-13 and abs(np.linalg.norm(ov[-nlast:]) - 1.0) <= 1e-13
    else:
        assert np.abs(ov).max() <= 1e-13
    # the sites are what the set-up says: B right-canonical, A left-canonical, U completes A
    for j in range(len(A)):
        b = B[j].reshape(B[j].shape[0], -1)
        a = A[j].reshape(-1, A[j].shape[2])
        assert np.abs(b @ b.conj().T - np.eye(b.shape[0])).max() <= 1e-13
        assert np.abs(a.conj().T @ a - np.eye(a.shape[1])).max() <= 1e-13
        if U[j] is not None and not (tr.CASES[case][3] and j == len(A) - 1):
            u = U[j].reshape(a.shape[0], -1)
            assert u.shape[1] == a.shape[0] - a.shape[1]
            assert np.abs(a.conj().T @ u).max() <= 1e-13


@pytest.mark.parametrize("case,kind", ALL)
def test_recursion_and_hdiag_against_dense(case, kind):
    A, B, U, W = tr.problem(case, kind)
    P = tr.dense_p(A, B, U)
    M = P.conj().T @ tr.dense_h(W) @ P
    n, nsite = M.shape[0], len(A)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if kind != "real" else 0)
    counts = {}
    y = tr.recursion(A, B, U, W, x, counts)
    scale = tr.hnorm_bound(W)
    err = np.abs(y - M @ x).max() / (np.linalg.norm(x) * scale)
    derr = np.abs(tr.hdiag(A, B, U, W) - np.diag(M).real).max() / scale
    print(f"{case}/{kind}: recursion {err:.2e}, hdiag {derr:.2e} of the scale; {counts}")
    assert err <= 1e-14 and derr <= 1e-14              # two orders inside the bound of the GPU test
    assert np.linalg.norm(M, 2) <= scale               # the scale bounds the operator
    assert counts["env"] <= 4 * (nsite - 1) and counts["heff"] <= 3 * nsite
    assert not np.any(tr.recursion(A, B, U, W, np.zeros(n)))


def test_case_table():
    """what the cases are meant to exercise"""
    shapes = {c: tr.xshapes(tr.problem(c, "real")[1], tr.problem(c, "real")[2]) for c in tr.CASES}
    assert shapes["edge"][0] is None and shapes["edge"][-1] == (8, 1)
    assert len(shapes["two_sites"]) == 2
    assert shapes["gap_site"][1] is None and shapes["gap_site"][2] is not None
    assert sum(s[0] * s[1] for s in shapes["bond17"] if s) == 475
    assert shapes["edge_psi0"][-1] == (9, 1)
