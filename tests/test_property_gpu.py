"""``Mps.mpo_expectations``, ``Property`` and the jobs that take one, on the GPU.

``mpo_expectations`` against ``expectations`` on the same state: the tolerance is the one of the existing comparisons
of a one-call route with its pinned per-site route, 1e-12 absolute (tests/test_site_rdms_gpu.py: ``site_expectations``
against ``expectations``; tests/test_charge_diffusion_gpu.py: ``edof_rdm`` against ``calc_edof_rdm``), relative to the
largest value of the list where that exceeds 1 (tests/test_site_rdms_gpu.py: ``site_rdms`` on a density operator)."""
import json
import os

import numpy as np
import pytest

from renormalizer_amd import HolsteinModel, Mol, Mpo, Phonon, Quantity
from renormalizer_amd.model.op import Op
from renormalizer_amd.property import Property, ops
from renormalizer_amd.utils import CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, constant

pytestmark = pytest.mark.gpu

ONE_CALL_TOL = 1e-12


def _agree(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    top = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(f"{what}: max |one call - pinned route| = {err:.2e}, largest value {np.abs(ref).max():.2e}")
    assert got.shape == ref.shape and err <= ONE_CALL_TOL * top, what


@pytest.fixture(scope="module")
def eng():
    from renormalizer_amd.engine import get_engine
    return get_engine()


@pytest.fixture(scope="module")
def model3():
    ph = Phonon.simple_phonon(Quantity(1400, "cm^{-1}"), Quantity(17, "a.u."), 4)
    return HolsteinModel([Mol(Quantity(3.87e-3, "a.u."), [ph])] * 3, Quantity(0.8, "eV"), 3)


def _operator_lists(model):
    n = model.mol_num
    lists = {"pairs": [Mpo(model, Op(r"a^\dagger a", [i, j])) for i in range(n) for j in range(n)],
             "x": ops.x_average(model)["x"],
             "S periodic": list(ops.e_ph_static_correlation(model, periodic=True).values())}
    local = []
    for imol in range(n):
        local += list(ops.e_ph_static_correlation(model, imol=imol).values())
    lists["S local"] = local
    return lists


@pytest.fixture(scope="module")
def states(model3):
    """the 3-molecule Holstein model as an Mps after two TDVP steps and as an MpDm after one thermal step"""
    from renormalizer_amd.mps import MpDm, thermal_state
    from renormalizer_amd.transport import ChargeDiffusionDynamics
    job = ChargeDiffusionDynamics(model3, evolve_config=EvolveConfig(EvolveMethod.tdvp_ps))
    job.evolve(2.0, 2)
    init = MpDm.max_entangled_ex(model3)
    init.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=8)
    init.evolve_config = EvolveConfig(EvolveMethod.tdvp_ps, adaptive=False, guess_dt=0.1 / 1j)
    rho, _ = thermal_state(init, Mpo(model3), Quantity(3000, "K").to_beta() / 2j, 1, auto_expand=True)
    assert job.latest_mps.is_complex and all(t.ndim == 4 for t in rho)
    return {"Mps": job.latest_mps, "MpDm": rho}


@pytest.mark.parametrize("kind", ("Mps", "MpDm"))
def test_mpo_expectations_against_expectations(eng, states, model3, kind):
    state = states[kind]
    for name, mpos in _operator_lists(model3).items():
        ref = state.expectations(mpos)
        s0 = eng.mps_expect_many_stats()
        got = state.mpo_expectations(mpos)
        s1 = eng.mps_expect_many_stats()
        assert s1["chain_kernel"] + s1["enqueued"] - s0["chain_kernel"] - s0["enqueued"] == 1
        assert s1["entries"] - s0["entries"] == len(mpos) and s1["sites"] - s0["sites"] == len(state)
        _agree(got, ref, f"{kind} {name}")
        assert got.dtype == ref.dtype
        assert np.abs(ref).max() > 1e-6                       # not a comparison of zeros
    # Op and OpSum are taken as expectations takes them; one operator is a call like any other; none is none
    one = [Op(r"a^\dagger a", 1)]
    _agree(state.mpo_expectations(one), [state.expectation(Mpo(model3, one[0]))], f"{kind} one Op")
    assert state.mpo_expectations([]).shape == (0,)
    # a scaled identity is its own window; the identity returns the squared norm of the site tensors' state
    ident = Mpo.identity(model3)
    _agree(state.mpo_expectations([ident, ident.scale(-0.5)]),
           [state.expectation(ident), state.expectation(ident.scale(-0.5))], f"{kind} identities")


# ---------------------------------------------------------------------------------------------- ThermalProp
NMOLS = 5


def _polaron_model():
    """the 5-molecule chain of the reference's polaron-structure test (Shi et al., J. Chem. Phys. 142, 174103)"""
    omega = 40.0 * constant.cm2au
    c = 3500.0 * constant.cm2au / (250.0 * constant.amu2au) ** 0.5 / constant.angstrom2au
    dis = c / omega ** 2
    j = 400 * constant.cm2au
    j_matrix = np.diag(np.ones(NMOLS - 1) * j, k=-1)
    j_matrix = j_matrix + j_matrix.T
    ph = Phonon([Quantity(omega), Quantity(omega)], [Quantity(0.0), Quantity(dis)], 5)
    return HolsteinModel([Mol(Quantity(0.0), [ph], 1.0)] * NMOLS, j_matrix)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "polaron_structure.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("periodic", (True, False))
def test_thermal_prop_with_properties(eng, golden, periodic):
    from renormalizer_amd.mps import MpDm, ThermalProp
    model = _polaron_model()
    if periodic:
        prop_mpos = ops.e_ph_static_correlation(model, periodic=True)
    else:
        prop_mpos = {}
        for imol in range(NMOLS):
            prop_mpos.update(ops.e_ph_static_correlation(model, imol=imol))
    prop_strs = list(prop_mpos) + ["e_rdm"]
    prop = Property(prop_strs, prop_mpos)
    beta = Quantity(1500.0, "K").to_beta()
    evolve_config = EvolveConfig(method=EvolveMethod.prop_and_compress, adaptive=True, adaptive_rtol=1e-4,
                                 guess_dt=0.1 / 1j)
    init = MpDm.max_entangled_ex(model)
    init.compress_config.threshold = 1e-4
    s0 = eng.mps_expect_many_stats()
    td = ThermalProp(init, evolve_config=evolve_config, properties=prop)
    td.evolve(beta / 2j, nsteps=1)
    s1 = eng.mps_expect_many_stats()
    # one engine call per recorded state for all the operators of the step
    assert s1["chain_kernel"] + s1["enqueued"] - s0["chain_kernel"] - s0["enqueued"] == 2
    assert s1["entries"] - s0["entries"] == 2 * len(prop_mpos)
    assert list(prop.prop_res) == prop_strs and len(prop_mpos) == (NMOLS if periodic else NMOLS ** 2)
    assert all(len(v) == 2 for v in prop.prop_res.values())
    assert td.e_occupations_array.shape == (2, NMOLS) and td.ph_occupations_array.shape == (2, NMOLS)
    assert len(td.energies) == 2 and td.vn_entropy_array.shape[0] == 2
    assert list(td.get_dump_dict())[5:] == prop_strs
    # the direct call reproduces what the job recorded for the same state
    prop.calc_properties(td.latest_mps, None)
    assert all(len(v) == 3 for v in prop.prop_res.values())
    _agree(prop.prop_res["e_rdm"][-1], prop.prop_res["e_rdm"][-2], "e_rdm, second call")
    for name in prop_mpos:
        assert prop.prop_res[name][-1] == prop.prop_res[name][-2]          # the same bits: a fixed summation order

    if periodic:
        corr = [prop.prop_res[f"S_{dis}_0"][-1] for dis in range(NMOLS)]
    else:
        corr = [sum(prop.prop_res[f"S_{i}_{(i + dis) % NMOLS}_0"][-1] for i in range(NMOLS)) for dis in range(NMOLS)]
    dev_rdm = np.abs(np.asarray(prop.prop_res["e_rdm"][-1]) - np.asarray(golden["e_rdm"])).max()
    dev_corr = np.abs(np.asarray(corr) - np.asarray(golden["e_ph_static_corr"])).max()
    print(f"periodic={periodic}: max |e_rdm - recorded| = {dev_rdm:.2e}, max |S(distance) - recorded| = {dev_corr:.2e}")
    print(f"S(distance) = {corr}")
    # the criterion of the reference's own test: numpy.allclose at its defaults
    assert np.allclose(prop.prop_res["e_rdm"][-1], golden["e_rdm"])
    assert np.allclose(corr, golden["e_ph_static_corr"])


# ---------------------------------------------------------------------------------------------- TransportKubo
def test_kubo_with_properties(eng):
    from test_kubo_gpu import _holstein_job
    from renormalizer_amd.transport.kubo import current_operators
    ph = Phonon.simple_phonon(Quantity(1), Quantity(1), 2)
    model = HolsteinModel([Mol(Quantity(0), [ph])] * 3, Quantity(1), 3)
    n_ops = [Mpo(model, Op(r"a^\dagger a", i)) for i in range(3)]
    j_oper = current_operators(model)[0]
    prop = Property(["n", "j"], {"n": n_ops, "j": j_oper})
    kubo, _, _ = _holstein_job(3, properties=prop)
    states = [kubo.latest_mps]
    for _ in range(2):
        kubo.evolve(nsteps=1, evolve_time=1)
        states.append(kubo.latest_mps)
    assert len(kubo.auto_corr) == 3 and len(prop.prop_res["n"]) == 3 and len(prop.prop_res["j"]) == 3
    assert np.asarray(prop.prop_res["n"]).shape == (3, 2, 3)
    assert list(kubo.get_dump_dict())[-2:] == ["n", "j"]
    # the last recorded step against the pinned routes on the same pair
    bra, ket = states[-1]
    _agree(prop.prop_res["n"][-1][0], bra.e_occupations, "n in the bra")
    _agree(prop.prop_res["n"][-1][1], ket.e_occupations, "n in the ket")
    _agree([prop.prop_res["j"][-1]], [ket.expectation(j_oper, bra)], "<bra| j |ket>")
