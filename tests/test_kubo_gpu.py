"""``TransportKubo`` on the GPU against exact current-current correlation functions.

The yardstick is numpy, inside this file: H and the number operators are ``Mpo(...).todense()`` (pinned to the
reference by the dense MPO tests), the current operators are commutators [P, H_part] (not the code under test),
everything is restricted to the one-exciton sector, and with H = U eps U^+, p the Boltzmann weights,

    C_XY(t) = - sum_ab p_a exp(i (eps_a - eps_b) t) X_ab Y_ba

(the sign: the operators are kept real, each lacks a factor -i).  Tolerance 5e-2 relative, the one of the reference's
own test; the reference itself deviates from these values by 9.0e-5 (Holstein, scheme 3), 3.6e-10 (scheme 4) and 2.7e-6
(Peierls, relative on the sum)."""
import os

import numpy as np
import pytest

from test_kubo_host import _comm, _number, _polarisation, peierls_ring, ring_commutator

pytestmark = pytest.mark.gpu


def _exact(h, n_op, pairs, temperature, times):
    """[C_XY(t) for (X, Y) in pairs] in the sector where n_op has eigenvalue 1"""
    occ = np.diag(n_op)
    assert np.allclose(n_op, np.diag(occ))
    idx = np.where(np.isclose(occ, 1.0))[0]
    hs = h[np.ix_(idx, idx)]
    eps, u = np.linalg.eigh(hs)
    p = np.exp(-temperature.to_beta() * (eps - eps.min()))
    p /= p.sum()
    t = np.asarray(times, dtype=float)
    phase = np.exp(1j * (eps[None, :, None] - eps[None, None, :]) * t[:, None, None])      # (t, a, b)
    out = []
    for x, y in pairs:
        xe, ye = u.conj().T @ x[np.ix_(idx, idx)] @ u, u.conj().T @ y[np.ix_(idx, idx)] @ u
        out.append(-np.einsum("a,tab,ab,ba->t", p, phase, xe, ye))
    return out


def _holstein(scheme):
    from renormalizer_amd import HolsteinModel, Mol, Phonon, Quantity
    ph = Phonon.simple_phonon(Quantity(1), Quantity(1), 2)
    return HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(1), scheme)


def _holstein_exact(model, temperature, times):
    from renormalizer_amd import Mpo
    h = Mpo(model).todense()
    j = _comm(_polarisation(model, [0, 1, 2]), h)
    n_op = sum(_number(model, m) for m in range(3))
    return _exact(h, n_op, [(j, j)], temperature, times)[0]


def _holstein_job(scheme, adaptive=True, **kw):
    from renormalizer_amd import CompressConfig, EvolveConfig, EvolveMethod, Quantity
    from renormalizer_amd.transport import TransportKubo
    from renormalizer_amd.utils import CompressCriteria
    model = _holstein(scheme)
    temperature = Quantity(50000, "K")
    compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=24)
    if adaptive:
        evolve_config = EvolveConfig(EvolveMethod.tdvp_ps, adaptive=True, guess_dt=0.5, adaptive_rtol=1e-3)
    else:
        evolve_config = EvolveConfig(EvolveMethod.tdvp_ps)
    ievolve_config = EvolveConfig(EvolveMethod.tdvp_ps, adaptive=True, guess_dt=-0.1j)
    return TransportKubo(model, temperature, compress_config=compress_config, ievolve_config=ievolve_config,
                         evolve_config=evolve_config, **kw), model, temperature


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


@pytest.mark.parametrize("scheme", (3, 4))
def test_holstein_kubo(eng, scheme, tmp_path):
    from renormalizer_amd.utils.constant import mobility2au
    s0 = eng.mps_sandwich_stats()
    kubo, model, temperature = _holstein_job(scheme, dump_dir=str(tmp_path), job_name="kubo")
    kubo.evolve(nsteps=5, evolve_time=5)
    s1 = eng.mps_sandwich_stats()
    exact = _holstein_exact(model, temperature, kubo.evolve_times_array)
    dev = np.abs(kubo.auto_corr - exact).max() / np.abs(exact).max()
    rel = np.abs(kubo.auto_corr - exact) / np.abs(exact)
    print(f"scheme {scheme}: C(t) = {kubo.auto_corr}, exact {exact}, max relative deviation {rel.max():.2e}")
    assert len(kubo.auto_corr) == 6 and kubo.j_oper2 is None
    assert np.allclose(kubo.auto_corr, exact, rtol=5e-2), f"max relative deviation {rel.max():.3e} ({dev:.3e} of max|C|)"
    # every recorded value came through the chain kernel: D = 24 with w <= 5 is inside the LDS rule
    assert s1["chain_kernel"] - s0["chain_kernel"] == 6 and s1["enqueued"] == s0["enqueued"]
    assert s1["sites"] - s0["sites"] == 6 * len(kubo.latest_mps.bra_mps)
    # mobility: the trapezoid of the recorded series over k_B T
    t, c = np.asarray(kubo.evolve_times, dtype=float), kubo.auto_corr.real
    trapezoid = sum((c[i] + c[i + 1]) * (t[i + 1] - t[i]) / 2 for i in range(len(t) - 1))
    au, cm2 = kubo.calc_mobility()
    assert np.isclose(au, trapezoid / temperature.as_au(), rtol=1e-13, atol=0) and np.isclose(cm2, au / mobility2au, rtol=1e-15)
    # the dump holds the reference's keys
    with np.load(tmp_path / "kubo.npz", allow_pickle=True) as f:
        assert sorted(f.files) == sorted(["mol list", "temperature", "time series", "auto correlation",
                                          "auto correlation decomposition", "mobility"])
        assert np.array_equal(f["auto correlation"], kubo.auto_corr) and float(f["mobility"]) == cm2
    # a second job with the same thermal dump reads the state instead of propagating: the same series bit for bit
    assert os.path.exists(tmp_path / "kubo_impdm.npz") and not kubo.thermal_state_loaded
    again, _, _ = _holstein_job(scheme, thermal_dump_path=str(tmp_path / "kubo_impdm.npz"))
    assert again.thermal_state_loaded
    again.evolve(nsteps=5, evolve_time=5)
    assert again.auto_corr.tobytes() == kubo.auto_corr.tobytes()


def test_lockstep_evolution_gives_the_bits_of_separate_evolves(eng):
    """fixed-step TDVP-PS: the three states qualify for ``evolve_batch``'s lock-step, which must reproduce ``evolve``"""
    from renormalizer_amd.transport.kubo import BraKetPairKubo
    kubo, model, temperature = _holstein_job(3, adaptive=False)
    bra, ket = kubo.latest_mps
    single = [kubo.auto_corr[0]]
    for _ in range(3):
        ket, bra = ket.evolve(kubo.h_mpo, 0.25), bra.evolve(kubo.h_mpo, 0.25)
        single.append(-BraKetPairKubo(bra, ket, kubo.j_oper).ft)
    kubo.evolve(evolve_dt=0.25, nsteps=3)
    assert kubo.auto_corr.tobytes() == np.array(single).tobytes()
    exact = _holstein_exact(model, temperature, kubo.evolve_times_array)
    rel = np.abs(kubo.auto_corr - exact) / np.abs(exact)
    assert np.allclose(kubo.auto_corr, exact, rtol=5e-2), f"max relative deviation {rel.max():.3e}"


def test_peierls_kubo(eng):
    from renormalizer_amd import CompressConfig, EvolveConfig, EvolveMethod, Mpo
    from renormalizer_amd.transport import TransportKubo
    from renormalizer_amd.utils import CompressCriteria
    n = 3
    model, hop, assisted, temperature = peierls_ring(n)
    compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=24)
    evolve_config = EvolveConfig(EvolveMethod.tdvp_ps, adaptive=True, guess_dt=50)
    ievolve_config = EvolveConfig(EvolveMethod.tdvp_ps, adaptive=True, guess_dt=-10j)
    s0 = eng.mps_sandwich_stats()
    kubo = TransportKubo(model, temperature, compress_config=compress_config, ievolve_config=ievolve_config,
                         evolve_config=evolve_config)
    kubo.evolve(nsteps=5, evolve_time=1000)
    s1 = eng.mps_sandwich_stats()
    print(f"current operators: MPO bonds {kubo.j_oper.bond_dims} and {kubo.j_oper2.bond_dims}")
    h = Mpo(model).todense()
    j1, j2 = ring_commutator(model, hop, n), ring_commutator(model, assisted, n)
    n_op = sum(_number(model, m) for m in range(n))
    pieces = np.array(_exact(h, n_op, [(j1, j1), (j1, j2), (j2, j1), (j2, j2)], temperature, kubo.evolve_times_array)).T
    total = pieces.sum(axis=1)
    got = kubo.auto_corr_decomposition
    assert got.shape == (6, 4) and np.array_equal(kubo.auto_corr, got[:, 0] + got[:, 1] + got[:, 2] + got[:, 3])
    for name, a, b in [(f"piece {k + 1}", got[:, k], pieces[:, k]) for k in range(4)] + [("sum", kubo.auto_corr, total)]:
        dev = np.abs(a - b).max() / np.abs(b[0])
        print(f"{name}: C(0) = {b[0]:.4e}, max |deviation| / |C(0)| = {dev:.2e}")
        assert np.all(np.abs(a - b) <= 5e-2 * np.abs(b[0])), f"{name}: deviation {dev:.3e} of |C(0)|"
    # four matrix elements per recorded step, all through the chain kernel
    assert s1["chain_kernel"] - s0["chain_kernel"] == 4 * 6 and s1["enqueued"] == s0["enqueued"]
