"""Pin of every contraction plan (renormalizer_amd/csrc/mpse_plans.h): tests/host_emu/plan_dump.cpp enumerates planner
calls and prints a hash of each plan's canonical dump; tests/golden/plan_pins.txt holds what the planners gave before
they were rewritten on labelled views.  A plan is a list of integers, so equal dumps mean the executors and the kernels
are handed the same work.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "plan_pins.txt")

# every branch the planners can take: the grid of the dump tool must reach each of them
TALLIES = ["unit_copy", "beta_source", "two_ranges", "kind_gemm", "kind_copy", "kind_wmix", "kind_ggemm",
           "env_wmix_taken", "env_wmix_refused", "epi", "split2", "direct_plane", "alias", "temporary", "second_r_launch"]
ERRORS = ["heff(0-site): wl != wr",
          "heff: nsite must be 0, 1 or 2",
          "fold: not a plain complex one-site centre with a real MPO site",
          "fold: centre too small or not tile aligned",
          "fold: too many channels",
          "fold: too many blocks per channel",
          "fold: blocks too large for the elementwise pass",
          "fold: the MPO site is zero",
          "env: bad domain",
          "env_multi: 1 to 4 MPO layers",
          "heff (two layers): one- or two-site centres only",
          "heff (two layers): bra bonds must equal ket bonds",
          "heff (two layers, 2-site): the batch index is danc1, danc must be 1",
          "heff_ft: empty extent",
          "heff_ft: a layer acts on MPSE_LEG_UP or MPSE_LEG_DOWN",
          "heff_ft: layers on different legs commute - give the one on the up leg first"]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pins") / "plan_dump")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(REPO, "tests", "host_emu", "plan_dump.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def lines(tool):
    return subprocess.check_output([tool], text=True).splitlines()


def test_every_plan_is_the_pinned_one(tool, lines):
    with open(GOLDEN) as f:
        want = [l.rstrip("\n") for l in f if not l.startswith("#")]
    assert len(want) > 4000
    for w, g in zip(want, lines):
        if w != g:
            key = g.split(" ")[0]
            dump = "" if g.startswith("tally") else subprocess.check_output([tool, "--case", key], text=True)
            pytest.fail("first difference from tests/golden/plan_pins.txt:\n  pinned %s\n  now    %s\n%s" % (w, g, dump))
    assert len(lines) == len(want)


def test_the_grid_reaches_every_branch(lines):
    tally = {}
    for l in lines:
        if l.startswith("tally error: "):
            name, n = l[len("tally "):].rsplit(" = ", 1)
            tally[name] = int(n)
        elif l.startswith("tally "):
            _, name, n = l.split(" ")
            tally[name] = int(n)
    for name in TALLIES + ["error: " + e for e in ERRORS]:
        assert tally.get(name, 0) > 0, name


def test_case_dump_names_every_field(tool):
    out = subprocess.check_output([tool, "--case", "fold.penta.d16.w4.u3.e1.r1"], text=True)     # epilogue mix, halved tiles
    out += subprocess.check_output([tool, "--case", "fold.second.d4.w4.u3.e0.r0"], text=True)    # elementwise pass
    for word in ("error=", "tmp=", "two_results=", "step kind=3", "scan_a on=1", "group nseg=", "seg a=", "epi src=", "dst ",
                 "term b=", "split2=1", "marks="):
        assert word in out, word
