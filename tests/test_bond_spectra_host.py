"""Host side of the Schmidt weights of the bonds (no GPU): the algebra of ``mpse_mps_bond_spectra`` restated in NumPy
(``gram_spectra`` of tests/bond_spectra_refs.py) against the reference's values and against the dense SVD, the path rule
of ``mpse_mps_bond_spectra_plan`` on dims tables, and the checks ``Engine.mps_bond_spectra`` makes before it calls the
library.

LDS plan (renormalizer_amd/csrc/mpse_bondspec.hip): the walks need region E, the largest D * (D | 1) over the bonds,
plus region T, the largest D_l * (D_r | 1) over the sites; the eigensolver 2 D (D | 1) + D at the largest bond, which is
never less; working elements of 8 (real) or 16 (complex) bytes."""
import os

import numpy as np
import pytest

from bond_spectra_refs import (decaying, dense_spectra, entropy, gram_spectra, padded,
                               state_with_spectrum)          # (tests/bond_spectra_refs.py)
from renormalizer_amd.engine import BOND_SPECTRA_PLAN_INFO, RDM1_PLAN_INFO, check_selection, mps_bond_spectra_plan


def _table(bonds, d=2, danc=1):
    return [[bonds[i], d, danc, bonds[i + 1]] for i in range(len(bonds) - 1)]


def test_gram_route_reproduces_the_reference(golden_dir):
    """bond_sv ** 2 to 1e-12 and bond_entropy to 1e-10, the project's tolerances for density matrices and entropies"""
    z = np.load(os.path.join(golden_dir, "observables_holstein_small.npz"))
    sites = [z[f"mps_site_{i}"] for i in range(int(z["mps_nsite"]))]
    p = gram_spectra(sites)
    ref = z["bond_sv"] ** 2
    assert np.abs(padded(p, ref.shape[1]) - ref).max() < 1e-12
    assert np.abs(np.array([entropy(r) for r in p]) - z["bond_entropy"]).max() < 1e-10
    assert np.abs(padded(dense_spectra(sites), ref.shape[1]) - ref).max() < 1e-12


@pytest.mark.parametrize("kind", ("real", "complex", "mixed"))
@pytest.mark.parametrize("bonds, d, cut", (((1, 2, 1), 2, 0), ((1, 3, 3, 1), 3, 1), ((1, 2, 4, 7, 4, 2, 1), 2, 2),
                                           ((1, 4, 16, 4, 1), 4, 1), ((1, 4, 17, 4, 1), 5, 1)))
def test_gram_route_against_the_dense_svd(bonds, d, cut, kind):
    rng = np.random.default_rng(4000 + max(bonds))
    sites = state_with_spectrum(rng, bonds, (d,) * (len(bonds) - 1), cut, decaying(bonds[cut + 1]), kind)
    assert np.iscomplexobj(sites[1]) == (kind != "real") and np.iscomplexobj(sites[0]) == (kind == "complex")
    dense, gram = dense_spectra(sites), gram_spectra(sites)
    assert np.abs(dense[cut][:bonds[cut + 1]] - decaying(bonds[cut + 1])).max() < 1e-13     # the builder did its job
    for k, (a, b) in enumerate(zip(dense, gram)):
        assert len(b) == bonds[k + 1]
        assert np.abs(padded([a], len(b))[0] - b).max() < 1e-13 and abs(entropy(a) - entropy(b)) < 1e-12


def test_plan_reports_its_limits():
    ok, info = mps_bond_spectra_plan(_table((1, 4, 4, 1)), 2, True)
    assert tuple(info) == BOND_SPECTRA_PLAN_INFO == RDM1_PLAN_INFO + ("eig_elems", "sweep_cap") and info["valid"] == 1
    assert info["lds_budget"] == 160 * 1024 and info["threads"] == 1024
    assert 1 <= info["bond_limit"] <= info["bond_fit_limit"] == 64
    assert info["nsel_limit"] == 0 and info["p_limit"] == 65536 and info["sweep_cap"] >= 2
    # by hand: E = 4 rows of pitch 5, T = 4 rows of pitch 5: the walks need 40 elements; the eigensolver two regions of
    # 4 x 5 and a strip of 4: 44 elements, the larger: complex 704 bytes, real 352
    assert info["e_elems"] == 20 and info["t_elems"] == 20 and info["eig_elems"] == 44 and info["lds_fit_bytes"] == 704
    assert ok == (info["bond_limit"] >= 4) and info["lds_bytes"] == (704 if ok else 0) and info["max_bond"] == 4
    ok_r, real = mps_bond_spectra_plan(_table((1, 4, 4, 1)), 2, False)
    assert real["lds_fit_bytes"] == 352 and real["lds_bytes"] == (352 if ok_r else 0) and ok_r == ok
    # bonds (1, 2, 6, 1): E = 6 * 7, T = max(1 * 3, 2 * 7, 6 * 1); eigensolver 2 * 42 + 6
    info = mps_bond_spectra_plan(_table((1, 2, 6, 1)), 1, True)[1]
    assert info["e_elems"] == 42 and info["t_elems"] == 14 and info["eig_elems"] == 90 and info["lds_fit_bytes"] == 90 * 16


@pytest.mark.parametrize("cplx", (False, True))
def test_bond_at_the_limit_and_above(cplx):
    es = 16 if cplx else 8
    limit = mps_bond_spectra_plan(_table((1, 1, 1)), 1, cplx)[1]["bond_limit"]
    ok, info = mps_bond_spectra_plan(_table((1, limit, limit, limit, 1)), 3, cplx)
    assert ok and info["max_bond"] == limit and info["eig_elems"] == 2 * limit * (limit | 1) + limit
    assert info["lds_bytes"] == info["eig_elems"] * es <= info["lds_budget"]
    ok, info = mps_bond_spectra_plan(_table((1, limit, limit + 1, limit, 1)), 3, cplx)
    assert not ok and info["valid"] == 1 and info["lds_bytes"] == 0 and info["max_bond"] == limit + 1
    fit = info["bond_fit_limit"]
    assert (info["lds_fit_bytes"] > 0) == (limit + 1 <= fit)
    ok, info = mps_bond_spectra_plan(_table((1, fit, fit, fit, 1)), 3, cplx)
    assert ok == (fit <= limit) and info["lds_fit_bytes"] == (2 * fit * (fit + 1) + fit) * es <= info["lds_budget"]
    assert info["e_elems"] == fit * (fit + 1)
    ok, info = mps_bond_spectra_plan(_table((1, fit, fit + 1, fit, 1)), 3, cplx)
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0 and info["e_elems"] == 0 and info["eig_elems"] == 0


def test_physical_extent_over_the_limit():
    assert mps_bond_spectra_plan(_table((1, 1, 1), d=65536), 1, False)[0]
    assert mps_bond_spectra_plan(_table((1, 1, 1), d=256, danc=256), 1, False)[0]
    for d, danc in ((65537, 1), (256, 257), (1, 65537)):
        ok, info = mps_bond_spectra_plan(_table((1, 1, 1), d=d, danc=danc), 1, False)
        assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0


def test_tables_that_are_no_chain():
    good = _table((1, 1, 1, 1))
    assert mps_bond_spectra_plan(good, 2, True)[0]
    for i, j, v in ((0, 0, 2), (2, 3, 2), (1, 0, 4), (1, 1, 0), (1, 2, 0), (2, 3, -1)):
        bad = [list(r) for r in good]
        bad[i][j] = v
        ok, info = mps_bond_spectra_plan(bad, 2, True)
        assert not ok and info["valid"] == 0 and info["max_bond"] == 0, bad
    assert not mps_bond_spectra_plan([], 1, True)[0] and mps_bond_spectra_plan([], 1, True)[1]["valid"] == 0


def test_selections_of_any_size_and_none():
    tab = _table((1,) + (1,) * 301 + (1,))          # 302 sites, 301 bonds
    ok, info = mps_bond_spectra_plan(tab, 300, True)
    assert ok and info["lds_fit_bytes"] == 3 * 16   # two 1 x 1 regions and a strip of 1
    ok, info = mps_bond_spectra_plan(tab, 0, True)   # an empty selection is refused
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0
    assert not mps_bond_spectra_plan(tab, -1, True)[0]
    ok, info = mps_bond_spectra_plan(_table((1, 1)), 1, True)     # a chain of one site has no bond
    assert not ok and info["valid"] == 1 and info["lds_fit_bytes"] == 0


def test_selection_is_checked_before_the_library():
    n = 6                                                           # six sites: the bonds 0 .. 4
    assert check_selection("mps_bond_spectra", (0, 3, 4), n - 1) == [0, 3, 4]
    for sel in ((5,), (0, 5), (2, 0), (1, 1), (-1, 1), (), (0, 2, 1)):
        with pytest.raises(ValueError):
            check_selection("mps_bond_spectra", sel, n - 1)
