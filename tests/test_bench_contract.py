"""The JSON line of bench.py as the driver reads it: the latest committed line (profiles/rNN_bench_20steps.json, printed
by `python bench.py --gpus 1 --steps 20 --warmup 5` on an MI355X) carries every field of the contract, is consistent with
itself, and names BASELINE.json's metric; bench.py accepts the driver's flags.  No GPU needed, except for the
small --dump-outputs run (pytest -m gpu)."""
import glob
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _latest_line():
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r[0-9][0-9]_bench_20steps.json")))
    assert files, "no committed bench line"
    with open(files[-1]) as fh:
        text = fh.read().strip()
    assert "\n" not in text, "the bench prints ONE line"
    return json.loads(text)


def test_bench_line_has_the_contract_fields():
    d = _latest_line()
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "c128" and d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5
    assert "workload" in d["config"] and "model" not in d["config"]
    nsite = d["config"]["nsite"]
    # one step = one evolve = 2 N site updates
    assert abs(d["value"] - 2 * nsite / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1
    assert r["traffic"] is None or r["traffic"] >= r["compulsory_bytes_per_launch"]
    c = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] in ("reference", "port") and c["unit"] == d["unit"] and c["value"] > 0
    dims = d["config"]["bond_dims"]
    assert len(dims) == nsite + 1 and all(x == d["config"]["bond_dim"] for x in dims[4:-4])


def test_bench_line_names_the_baseline_metric():
    """BASELINE.json: "DMRG/TDVP sweep sites/sec at (Nsite, Dbond, dphys); % MFMA roofline" - the line quotes sweep
    site updates per second at the named (Nsite, Dbond, dphys) and carries the MFMA roofline fraction."""
    d = _latest_line()
    with open(os.path.join(REPO, "BASELINE.json")) as fh:
        base = json.load(fh)
    assert "sweep" in base["metric"] and "Nsite" in base["metric"] and "MFMA" in base["metric"]
    assert "TDVP" in d["metric"] and "sweep" in d["metric"] and "/sec" in d["metric"]
    assert all(k in d["metric"] for k in ("Nsite=", "Dbond=", "dphys="))
    assert d["roofline"]["bound"] == "mfma"


def test_bench_accepts_the_driver_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in out.stdout


def test_bench_offers_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_bench_dump_outputs_small_chain(tmp_path):
    """A small chain through the timed path: --steps sets the timed steps, the line carries ms_per_step, and
    --dump-outputs writes the evolved state as float64 .npy files (normalised occupations, one file per site)."""
    import numpy as np
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--cpu-updates", "0", "--nmol", "3", "--pdim", "4", "--bond-dim", "16", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    files = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    nsite = d["config"]["nsite"]
    assert {"e_occupations", "energy", "bond_dims", "coeff", "site_shapes"} <= set(files)
    assert sorted(k for k in files if k.startswith("site_") and k != "site_shapes") == [f"site_{i:03d}" for i in range(nsite)]
    assert all(a.dtype == np.float64 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["bond_dims"].tolist() == d["config"]["bond_dims"]
    assert abs(files["e_occupations"].sum() - 1.0) < 1e-9
    for i in range(nsite):
        assert files[f"site_{i:03d}"].shape == tuple(files["site_shapes"][i].astype(int)) + (2,)
