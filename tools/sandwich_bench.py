#!/usr/bin/env python3
"""Times <bra| O |ket> of density-operator chains three ways on one GPU: ``Mps.matrix_element`` through the chain kernel
(MPSE_SANDWICH_CHAIN=1: every chain whose launch fits, whatever its work), through the enqueued environment updates
(MPSE_SANDWICH_CHAIN=0), and ``ket.expectation(mpo, bra.conj())``, the path it replaces.

    python tools/sandwich_bench.py [out.md] [--quick]

The parent starts one child process per (variant, round), the two ``matrix_element`` variants alternating, each under
its own time limit; a child warms every shape up and then repeats the call until the timed window exceeds a second.
Every figure is a host clock around calls that end in the engine's own read-back.  Shapes: MpDm chains of 10 and 40
sites, electron sites d = danc = 2 alternating with phonon sites d = danc = p, p = 2 / 4 / 10, bonds 16 / 24 / 32 / 48,
a sparse real MPO with 3 or 5 channels (the shape of a current operator), complex states from a fixed seed.

From the table the tool derives the work bound of ``mpse_mps_sandwich_plan``: the largest multiply-add count of a
heaviest site up to which the chain kernel is not slower than the enqueued path for EVERY measured shape at or below
it, rounded down to a power of two."""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS = 2
WINDOW = 1.0          # seconds a timed window has to exceed
CHILD_LIMIT = 900     # seconds per child


def shapes(quick):
    out = []
    for nsite in ((10,) if quick else (10, 40)):
        for p in (2, 4, 10):
            for D in ((16, 32) if quick else (16, 24, 32, 48)):
                for w in (3, 5):
                    out.append((nsite, p, D, w))
    return out


def build(shape, eng):
    """(bra, ket, mpo sites) of one shape: normalised random complex sites, a sparse real MPO"""
    from renormalizer_amd.mps.mpdm import MpDm
    nsite, p, D, w = shape
    rng = np.random.default_rng(hash(shape) % (2 ** 32))
    ds = [2 if i % 2 == 0 else p for i in range(nsite)]
    bonds = [1] + [min(D, 4 ** min(i, nsite - i)) for i in range(1, nsite)] + [1]
    wb = [1] + [w] * (nsite - 1) + [1]
    states = []
    for _ in range(2):
        m = MpDm()
        m._mp = []
        for i, d in enumerate(ds):
            a = rng.standard_normal((bonds[i], d, d, bonds[i + 1])) + 1j * rng.standard_normal((bonds[i], d, d, bonds[i + 1]))
            m._mp.append(eng.asdevice(a / np.linalg.norm(a) * np.sqrt(bonds[i + 1])))
        m.dtype = np.dtype(np.complex128)
        m.qntot = np.zeros(1, dtype=int)       # (what ``conj`` copies)
        states.append(m)
    ws = []
    for i, d in enumerate(ds):
        m = np.zeros((wb[i], d, d, wb[i + 1]))
        for g in range(wb[i]):
            for f in range(wb[i + 1]):
                if g == f or f == 0 or g == wb[i] - 1:        # pass-through channels and the operator columns
                    m[g, :, :, f] = np.eye(d) if g == f else np.diag(rng.standard_normal(d - 1), 1) + np.diag(rng.standard_normal(d - 1), -1)
        ws.append(m)
    return states[0], states[1], ws


class _W:
    """the MPO sites with the interface ``Mps.matrix_element`` and ``Environ`` read"""

    def __init__(self, eng, ws):
        self.ws, self.dev = ws, [eng.asdevice(m) for m in ws]

    def __len__(self):
        return len(self.ws)

    def __getitem__(self, i):
        return self.ws[i]

    def device(self, i, eng):
        return self.dev[i]


def child(variant, quick):
    from renormalizer_amd.engine import get_engine, mps_sandwich_plan
    eng = get_engine()
    for shape in shapes(quick):
        bra, ket, ws = build(shape, eng)
        mpo = _W(eng, ws)
        if variant == "expectation":
            def fn():
                return complex(ket.expectation(mpo, bra.conj()))
        else:
            def fn():
                return bra.matrix_element(mpo, ket, self_is_conj=False)
        s0 = eng.mps_sandwich_stats()
        t0 = time.perf_counter()
        val = fn()
        fn()
        warm = (time.perf_counter() - t0) / 2
        s1 = eng.mps_sandwich_stats()
        reps = max(3, int(np.ceil(1.1 * WINDOW / max(warm, 1e-6))))
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        eng.sync()
        window = time.perf_counter() - t0
        dims = eng.sandwich_dims(bra._mp, mpo.dev, ket._mp)
        info = mps_sandwich_plan(dims, True)[1]
        path = "-" if variant == "expectation" else ("chain" if s1["chain_kernel"] > s0["chain_kernel"] else "enqueued")
        print("ROW " + json.dumps({"variant": variant, "shape": shape, "path": path, "seconds": window / reps, "reps": reps,
                                   "window": window, "work": info["work"],
                                   "value": [val.real, val.imag]}), flush=True)


def run_child(variant, quick):
    env = dict(os.environ)
    env.pop("MPSE_SANDWICH_CHAIN", None)
    if variant != "expectation":
        env["MPSE_SANDWICH_CHAIN"] = "1" if variant == "chain" else "0"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant] + (["--quick"] if quick else [])
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
    if res.returncode != 0:
        raise RuntimeError(f"child {variant} ended with {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]


def work_bound(rows):
    """largest power of two W with chain <= enqueued for every measured shape of work <= W that the kernel took; None:
    no shape at all"""
    pts = sorted((r["work"], r["chain"] <= r["enqueued"]) for r in rows if r["path"] == "chain")
    best = None
    for work, ok in pts:
        if not ok:
            break
        best = work
    return None if best is None else 1 << (int(best).bit_length() - 1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1], quick)
        return
    out_path = args[0] if args else None
    times = {}
    meta = {}
    order = [v for _ in range(ROUNDS) for v in ("chain", "enqueued")] + ["expectation"]
    for variant in order:
        for r in run_child(variant, quick):
            key = tuple(r["shape"])
            times.setdefault(key, {}).setdefault(variant, []).append(r["seconds"])
            m = meta.setdefault(key, {"work": r["work"], "values": {}})
            if variant == "chain":
                m["path"] = r["path"]
            m["values"][variant] = complex(*r["value"])
        print(f"child {variant} done", flush=True)
    lines = [f"{ROUNDS} rounds per `matrix_element` variant in alternating child processes, 1 of `expectation`; every "
             f"window > {WINDOW:.0f} s after a warm-up; median (min, max) per call", "",
             "| sites | phonon d | bond | MPO bond | work of the heaviest site | kernel path | chain kernel | enqueued updates | "
             "`expectation(mpo, bra.conj())` | chain / enqueued |", "|---|---|---|---|---|---|---|---|---|---|"]

    def fmt(ts):
        ts = np.array(ts) * 1e6
        return f"{np.median(ts):.1f} us ({ts.min():.1f}, {ts.max():.1f})"

    rows = []
    for key in sorted(times, key=lambda k: (meta[k]["work"], k)):
        t, m = times[key], meta[key]
        v = m["values"]
        scale = max(abs(v["expectation"]), 1e-300)
        assert abs(v["chain"] - v["expectation"]) <= 1e-9 * scale and abs(v["enqueued"] - v["expectation"]) <= 1e-9 * scale, v
        c, e = float(np.median(t["chain"])), float(np.median(t["enqueued"]))
        rows.append({"work": m["work"], "path": m["path"], "chain": c, "enqueued": e})
        lines.append(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]} | {m['work']:.3g} | {m['path']} | {fmt(t['chain'])} | "
                     f"{fmt(t['enqueued'])} | {fmt(t['expectation'])} | {c / e:.2f} |")
    bound = work_bound(rows)
    lines += ["", f"work bound derived from this table: {bound} (2^{bound.bit_length() - 1})" if bound else
              "work bound: the chain kernel won at no measured shape"]
    text = "\n".join(lines) + "\n"
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
