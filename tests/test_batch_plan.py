"""plan_batch (csrc/gpsbb.hip) decides for every case of a fixed matrix exactly what batch set-up decided before planning became a
function of its own: gpsbb_test_plan's scalars and image hashes against tests/golden/batch_plans.json, which was recorded from the
commit before: tools/experiments/plan_dump_parent.patch prints the same values at the end of its batch_setup, which ran once per
set-up on a fresh batch, a ring's pushes with the carry the push before left.  (That record was taken on a CPU, the HIP calls of
that batch_setup compiled out — the decisions never depended on them; it is to be taken again on an MI355X through
gpsbb_batch_create and a ring of depth 2, which the patch serves as it is.)  No GPU here: the plan is plain arithmetic.

What each axis of the matrix (tests/batch_plan_cases.py) is there for, by the step of plan_batch it reaches:
  25M / 2M6 / 1M geometries        plan_kernel: the model kernels render the first two and decline 1 MS/s (ev); ev_state_log2
  mix (fs = 15.5 * 1.023 MHz + 20) plan_kernel: ev_dense without ev_all_dense, and FIXED sent to the stepped kernel for it
  t1075 / t1024 / t1023            plan_segments: indep_ok, CHAIN_INDEP_MIN_TILES from both sides
  t15 / t16 / t31 / t32, odd       plan_segments: n_cap = ntiles / CHAIN_SEG_MIN_TILES; a last tile that is not full
  16 x {1, 4, 5}                   host_seeding_wanted: 64 against 80 block-channels; `chained` needs two blocks or a carry
  16 x 400                         plan_seed_order's counting sort over thousands of chains; nsets; lap_bound's lane units
  segs-*                           plan_segments: fix_wg at nblocks * nseg = 2048, chain_model at CHAIN_MODEL_MAX_SEGS = 4096
  flags 0 / CHAIN / FIXED / both   plan_placement's `chained`, plan_fixed_point, plan_chain's host-side chain
  seed_where, chain_where, kernel  plan_laps_admit, host_seeding_wanted, chain_dev, chain_fix_seq, chain_starts, chain_model
  idle / zero / neg / tiny         row_off's idle entries, prev_prn reset; lap_eligible's step of zero and of 0 < |s| < 2^-50;
                                   by_sign in plan_carr_sorted
  gain-under / gain-over           ev_plan's amp_sum < 32768 (sum of 512 |gain| + 1)
  ring-carry                       the stream's carry: plan_placement with a carry, carry_phase in and out, cont0_mask (third push: a
                                   PRN swapped), both pre-passes and both kernels; 2x4: the small push the laps keep on the device
  ring-fixed / ring-plain          fixed_prev_* in plan_fixed_point; one table set per ring slot (max_sets)
  err-*                            plan_begin's three errors, the 32-bit tile-index limit at its first refused count
"""
import json
import os

import numpy as np
import pytest

import batch_plan_cases as bpc
from conftest import GOLDEN, load_package

GOLDEN_FILE = os.path.join(GOLDEN, "batch_plans.json")


def plan_case(pkg, case):
    """gpsbb_test_plan over the pushes of one case: [values per push], or the error code"""
    got = []
    ring = case["stream"] is not None
    prn = np.zeros(pkg.MAX_CHAN, np.int32)
    rough = np.zeros(pkg.MAX_CHAN, np.float64)
    fx = None
    for ch in case["ch"]:
        kw = dict(seed_where=case["seed_where"], synth_kernel=case["synth_kernel"], chain_where=case["chain_where"],
                  max_sets=1 if ring else 6)
        if case["stream"] == "carry":
            kw.update(carry_prn=prn, carry_phase=rough)
        if case["stream"] == "fixed" and fx is not None:
            kw.update(fixed_prev_prn=fx[0], fixed_prev_phase=fx[1])
        rc, v = pkg.plan(ch, case["delt"], case["nsamp"], case["flags"], **kw)
        if rc != 0:
            return rc
        got.append([v[f] for f in pkg.PLAN_FIELDS])
        nch = ch.shape[1]
        prn[:nch] = np.maximum(ch["prn"][-1], 0)
        if case["stream"] == "fixed":
            fx = bpc.fixed_chain_state(ch, case["delt"], case["nsamp"], True, *(fx or (None, None)))
    return got


@pytest.fixture(scope="module")
def matrix():
    pkg = load_package()
    pkg.build()
    with open(GOLDEN_FILE) as f:
        golden = json.load(f)
    return pkg, bpc.cases(pkg), golden


def test_matrix_is_the_recorded_one(matrix):
    pkg, cases, golden = matrix
    assert golden["fields"] == list(pkg.PLAN_FIELDS)
    assert [c["name"] for c in cases] == list(golden["cases"])
    assert 200 <= len(cases)


def test_plan_matches_parent(matrix):
    pkg, cases, golden = matrix
    wrong = []
    for case in cases:
        want = golden["cases"][case["name"]]
        got = plan_case(pkg, case)
        if case["expect"] is not None:
            assert want == case["expect"], case["name"]
        if got != want:
            if isinstance(got, list) and isinstance(want, list):
                diff = sorted({f for g, w in zip(got, want) for f, a, b in zip(pkg.PLAN_FIELDS, g, w) if a != b})
                wrong.append((case["name"], diff))
            else:
                wrong.append((case["name"], got if not isinstance(got, list) else "ok", want if not isinstance(want, list) else "ok"))
    assert not wrong, "%d of %d cases differ from the recorded plans: %r" % (len(wrong), len(cases), wrong[:20])
