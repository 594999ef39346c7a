#!/usr/bin/env python3
"""Times <bra|ket> three ways on one GPU: ``Mps.dot`` (two host-driven products per site), ``Mps.overlap`` through the
chain kernel, and ``Mps.overlap`` through the enqueued products (MPSE_OVERLAP_CHAIN=0), alternating, three repeats each
after a warm-up; every figure is a host clock around calls that end in the engine's own read-back.

    python tools/overlap_bench.py [out.md]

Cases: (a) the Holstein test model (3 molecules x 2 modes) at D = 10 and D = 32, (b) the 497-site thermofield FMO chain
of examples/fmo.py at D = 32, (c) dense random sites with the shapes of the benchmark chain (25 molecules, 16 phonon
levels) at D = 256, which is above the chain kernel's bond limit.  (a) and (b) are a real bra and the ket one TDVP-PS
step later; for them the share of one recorded spectra step (evolve + overlap) that the overlap takes is reported too."""
import importlib.util
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from renormalizer_amd import (CompressConfig, CompressCriteria, EvolveConfig, EvolveMethod, HolsteinModel, Mol, Mpo, Mps,  # noqa: E402
                              Phonon, Quantity)
from renormalizer_amd.engine import get_engine  # noqa: E402
from renormalizer_amd.utils import constant  # noqa: E402

REPEATS = 3


def holstein_test_model():
    omega = [Quantity(106.51, "cm^{-1}"), Quantity(1555.55, "cm^{-1}")]
    dis = [Quantity(30.1370), Quantity(8.7729)]
    ph_list = [Phonon.simple_phonon(o, d, 4) for o, d in zip(omega, dis)]
    j = np.array([[0.0, -0.1, -0.2], [-0.1, 0.0, -0.3], [-0.2, -0.3, 0.0]]) / constant.au2ev
    return HolsteinModel([Mol(Quantity(2.67, "eV"), ph_list, 15.45)] * 3, j, 3)


def fmo_chain():
    spec = importlib.util.spec_from_file_location("fmo_example", os.path.join(REPO, "examples", "fmo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.fmo_model(35, temperature_k=77.0)


def pair_one_step_apart(model, D, dt):
    """an exciton created on the centre molecule, expanded to bond dimension D (bra: real), and the same state one
    TDVP-PS step later (ket: complex); also returns what a further step needs"""
    psi = Mpo.onsite(model, r"a^\dagger", dof_set={model.mol_num // 2}).apply(Mps.ground_state(model, False))
    mpo = Mpo(model, offset=Quantity(psi.expectation(Mpo(model))))
    psi.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=D)
    psi.evolve_config = EvolveConfig(EvolveMethod.tdvp_ps)
    bra = psi.expand_bond_dimension(mpo).canonicalise()
    ket = bra.evolve(mpo, dt)
    return bra, ket, mpo


def dense_pair(nmol, pdim, D, rng):
    eng = get_engine()
    ps = [2, pdim] * nmol
    bonds = [1] + [min(D, 4 ** min(i, len(ps) - i)) for i in range(1, len(ps))] + [1]
    out = []
    for cplx in (False, True):
        m = Mps()
        sites = []
        for i, p in enumerate(ps):
            a = rng.standard_normal((bonds[i], p, bonds[i + 1]))
            if cplx:
                a = a + 1j * rng.standard_normal(a.shape)
            sites.append(eng.asdevice(a / np.linalg.norm(a) * np.sqrt(bonds[i + 1])))
        m._mp = sites
        m.dtype = np.dtype(np.complex128 if cplx else np.float64)
        out.append(m)
    return out


def timed(fn, inner):
    get_engine().sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        val = fn()
    get_engine().sync()
    return (time.perf_counter() - t0) / inner, val


def overlap_forced(bra, ket):
    os.environ["MPSE_OVERLAP_CHAIN"] = "0"
    try:
        return bra.overlap(ket, self_is_conj=False)
    finally:
        del os.environ["MPSE_OVERLAP_CHAIN"]


def measure(bra, ket, inner):
    """{name: [seconds per call] * REPEATS}, the three variants alternating inside every repeat"""
    eng = get_engine()
    variants = {"dot": lambda: bra.dot(ket, self_is_conj=False),
                "overlap": lambda: bra.overlap(ket, self_is_conj=False),
                "enqueued": lambda: overlap_forced(bra, ket)}
    s0 = eng.mps_overlap_stats()
    vals = {k: timed(f, 2)[1] for k, f in variants.items()}            # warm-up of every shape
    s1 = eng.mps_overlap_stats()
    path = "chain kernel" if s1["chain_kernel"] - s0["chain_kernel"] == 2 else "enqueued"
    assert s1["enqueued"] - s0["enqueued"] >= 2
    scale = max(abs(vals["dot"]), 1e-300)
    assert abs(vals["overlap"] - vals["dot"]) <= 1e-9 * scale and abs(vals["enqueued"] - vals["dot"]) <= 1e-9 * scale, vals
    times = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, f in variants.items():
            times[k].append(timed(f, inner)[0])
    return times, path


def fmt(ts):
    ts = np.array(ts) * 1e6
    return f"{np.median(ts):9.1f} us (min {ts.min():.1f}, max {ts.max():.1f})"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    eng = get_engine()
    lines = [f"device: {eng.device_name}; {REPEATS} repeats per figure, median (min, max); the variants alternate", ""]
    lines += ["| case | sites | max bond | path of `overlap` | `Mps.dot` | `Mps.overlap` | enqueued path | evolve step | "
              "overlap share of a step: dot -> overlap |", "|---|---|---|---|---|---|---|---|---|"]
    cases = [("(a) Holstein test model, D = 10", holstein_test_model, 10, 30.0, 200),
             ("(a) Holstein test model, D = 32", holstein_test_model, 32, 30.0, 200),
             ("(b) FMO thermofield chain, D = 32", fmo_chain, 32, 160.0, 5)]
    for name, build, D, dt, inner in cases:
        bra, ket, mpo = pair_one_step_apart(build(), D, dt)
        times, path = measure(bra, ket, inner)
        ev = [timed(lambda: ket.evolve(mpo, dt), 1)[0] for _ in range(REPEATS + 1)][1:]
        e = np.median(ev)
        share = [np.median(times[k]) / (e + np.median(times[k])) for k in ("dot", "overlap")]
        lines.append(f"| {name} | {len(ket)} | {max(ket.bond_dims)} | {path} | {fmt(times['dot'])} | {fmt(times['overlap'])} | "
                     f"{fmt(times['enqueued'])} | {e * 1e3:.2f} ms | {100 * share[0]:.2f} % -> {100 * share[1]:.2f} % |")
        print(lines[-1], flush=True)
    bra, ket = dense_pair(25, 16, 256, np.random.default_rng(5))
    times, path = measure(bra, ket, 20)
    lines.append(f"| (c) benchmark chain shapes, D = 256, dense random | {len(ket)} | 256 | {path} | {fmt(times['dot'])} | "
                 f"{fmt(times['overlap'])} | {fmt(times['enqueued'])} | - | - |")
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
