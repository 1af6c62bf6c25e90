"""plan_chain_only (csrc/gpsbb_plan.h) decides for every case of a fixed matrix exactly what gpsbb_chain_carrier decided inside its
own body before its plan became a function: gpsbb_test_chain_plan's values against tests/golden/chain_plans.json, which was
recorded from the commit before with tools/experiments/chain_plan_dump_parent.patch — that gpsbb_chain_carrier prints, at each
sub-batch of either path, b0, nb, cont0_mask and the hash of chunk0, and the hashes of h_cd and h_start0 as uploaded.  (The record
was taken on a CPU, the HIP calls of that function compiled out: its decisions never depended on them.)  No GPU here.

The sub-batch limits are knobs of the experiments build, read once per process: each limits group (tests/chain_plan_cases.py) runs
in a child process of its own.  What each case is there for:
  laps-8000x16     the running lap count against CHAIN_ONLY_LAPS = 6.0e6 (crossed twice), with the unit of a batch one block larger
  blocks-16424x5   CHAIN_ONLY_BLOCKS = 16384 cuts, the laps do not
  edges-*          lowered limits: a PRN that changes on a piece's first block, a channel idle across a boundary or on a piece's last
                   block, a zero and a negative step (cont0_mask, h_start0); -tiny: 0 < |step| < 2^-50 sends every piece to the row
                   walks; -long: the lowered lap limit cuts, not the block limit
  sw0 / sw1        the handle's GPSBB_OPT_SEED_WHERE: the library's choice, the row walks
  err-* / ok-*     the argument checks and the descriptor check (chain_only_chan_ok): prn, f_carr, carr_phase, the step's eighth —
                   and no code field
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_plan_cases as cpc
from conftest import GOLDEN, ROOT, load_package

GOLDEN_FILE = os.path.join(GOLDEN, "chain_plans.json")
LAP_UNIT_CARR = 4


@pytest.fixture(scope="module")
def matrix():
    """(package, cases, {name: what gpsbb_test_chain_plan gave}, the record)"""
    pkg = load_package()
    pkg.build()
    got = {}
    for group in cpc.LIMITS:
        env = dict(os.environ, **(cpc.LOWERED if group == "lowered" else {}))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_plan_cases.py"), "--plan", group], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got.update(json.loads(r.stdout.strip().splitlines()[-1]))
    with open(GOLDEN_FILE) as f:
        golden = json.load(f)
    return pkg, cpc.cases(pkg), got, golden


def test_matrix_is_the_recorded_one(matrix):
    _, cases, got, golden = matrix
    assert [c["name"] for c in cases] == list(golden["cases"]) and set(got) == set(golden["cases"])
    assert {c["limits"] for c in cases} == set(cpc.LIMITS)


def test_plan_matches_parent(matrix):
    _, cases, got, golden = matrix
    for c in cases:
        want = golden["cases"][c["name"]]
        if c["expect"] is not None:
            assert want == c["expect"], c["name"]
        else:
            assert isinstance(want, dict), c["name"]
        assert got[c["name"]] == want, c["name"]


def lap_unit(nbc):
    """lap_unit(NCO_CARR, nbc) of csrc/gpsbb.hip"""
    return 1 if nbc <= 256 else (min(LAP_UNIT_CARR, 2) if nbc <= 1024 else LAP_UNIT_CARR)


def running_laps(c, b0, nb):
    """a piece's lap count as the partition counts it: block j with the unit of a batch of j + 1 blocks"""
    ch = c["ch"][b0:b0 + nb]
    unit = np.array([lap_unit((j + 1) * ch.shape[1]) for j in range(nb)], np.float64)[:, None]
    laps = np.floor((np.floor(c["nsamp"] * np.abs(ch["f_carr"] * c["delt"])) + 1.0) / unit) + 3.0
    return float(np.sum(np.where(ch["prn"] > 0, laps, 0.0)))  # (sums of small integers: exact in any order)


def test_pieces_tile_the_blocks_within_the_limits(matrix):
    pkg, cases, got, _ = matrix
    for c in cases:
        v = got[c["name"]]
        if not isinstance(v, dict):
            continue
        max_blocks, max_laps = cpc.LIMITS[c["limits"]]
        assert v["npieces"] == len(v["pieces"]) <= pkg.CHAIN_PLAN_PIECES, c["name"]
        at = 0
        for b0, nb, cont0, chunk0 in v["pieces"]:
            assert b0 == at and 1 <= nb <= max_blocks, (c["name"], b0, nb)
            assert (chunk0 != 0) == bool(v["laps"]), c["name"]
            if v["laps"] and nb > 1:
                assert running_laps(c, b0, nb) <= max_laps, (c["name"], b0, nb)
            prn = c["ch"]["prn"]
            want = sum(1 << i for i in range(prn.shape[1]) if b0 > 0 and prn[b0, i] > 0 and prn[b0, i] == prn[b0 - 1, i])
            assert cont0 == want, (c["name"], b0)
            at += nb
        assert at == c["ch"].shape[0], c["name"]


def test_which_limit_cuts_and_which_path(matrix):
    _, cases, got, _ = matrix
    by = {c["name"]: c for c in cases}
    for name, v in got.items():
        if not isinstance(v, dict):
            continue
        c = by[name]
        assert v["laps"] == int(c["seed_where"] != 1 and "tiny" not in name), name
        if c["limits"] == "lowered":
            assert v["npieces"] >= 3, name
    nbs = lambda name: [p[1] for p in got[name]["pieces"]]
    assert len(nbs("laps-8000x16-sw0")) >= 3 and max(nbs("laps-8000x16-sw0")) < 16384  # the lap limit, twice or more
    assert nbs("laps-8000x16-sw1") == [8000]
    assert nbs("blocks-16424x5-sw0") == nbs("blocks-16424x5-sw1") == [16384, 40]
    assert nbs("edges-50x5-sw0") == nbs("edges-50x5-sw1") == nbs("edges-long-50x5-sw1") == [16, 16, 16, 2]
    assert max(nbs("edges-long-50x5-sw0")) < 16  # the lap limit
