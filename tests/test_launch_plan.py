"""plan_launch (csrc/gpsbb_plan.h) decides for every case of a fixed matrix exactly what the launch path decided while its decisions
still stood between its HIP calls: gpsbb_test_launch_plan's fields and kernel list against tests/golden/launch_plans.json, recorded
from the commit before (tools/experiments/launch_dump_parent.patch: that commit's batch_launch run on a CPU, the HIP calls not
evaluated, every kernel launch written down with its geometry, and the handle's last_* values afterwards).  No GPU here.

The matrix is tests/batch_plan_cases.py's, every set-up at 256 and 8 CUs, without and with the blocks' digests, a few also with the
pre-pass skipped (tests/launch_plan_cases.py).  Besides the record, properties that hold whatever it says."""
import json
import os

import numpy as np
import pytest

import batch_plan_cases as bpc
import launch_plan_cases as lpc
from conftest import GOLDEN, load_package

GOLDEN_FILE = os.path.join(GOLDEN, "launch_plans.json")


def launch_case(pkg, case):
    """gpsbb_test_launch_plan over the pushes and variants of one case: [[values per variant] per push], or the error code"""
    got = []
    prn = np.zeros(pkg.MAX_CHAN, np.int32)
    rough = np.zeros(pkg.MAX_CHAN, np.float64)
    fx = None
    for ch in case["ch"]:
        kw = dict(seed_where=case["seed_where"], synth_kernel=case["synth_kernel"], chain_where=case["chain_where"],
                  max_sets=1 if case["stream"] is not None else 6)
        if case["stream"] == "fixed" and fx is not None:
            kw.update(fixed_prev_prn=fx[0], fixed_prev_phase=fx[1])
        per_variant = []
        for cus, dg, skip in lpc.variants(case):
            if case["stream"] == "carry":  # (every variant plans the same push: from the same rough phases)
                kw.update(carry_prn=prn, carry_phase=rough.copy())
            rc, v = pkg.launch_plan(ch, case["delt"], case["nsamp"], case["flags"], cus=cus, want_digest=dg, skip=skip, **kw)
            if rc != 0:
                return rc
            per_variant.append(v)
        if case["stream"] == "carry":
            pkg.plan(ch, case["delt"], case["nsamp"], case["flags"], carry_prn=prn, carry_phase=rough,
                     **{k: kw[k] for k in ("seed_where", "synth_kernel", "chain_where", "max_sets")})
        got.append(per_variant)
        prn[:ch.shape[1]] = np.maximum(ch["prn"][-1], 0)
        if case["stream"] == "fixed":
            fx = bpc.fixed_chain_state(ch, case["delt"], case["nsamp"], True, *(fx or (None, None)))
    return got


def as_row(pkg, v):
    return [v[f] for f in pkg.LAUNCH_FIELDS] + [len(v["kernels"])] + [x for k in v["kernels"] for x in k]


@pytest.fixture(scope="module")
def matrix():
    pkg = load_package()
    pkg.build()
    with open(GOLDEN_FILE) as f:
        golden = json.load(f)
    cases = bpc.cases(pkg)
    return pkg, cases, golden, {c["name"]: launch_case(pkg, c) for c in cases}


def test_matrix_is_the_recorded_one(matrix):
    pkg, cases, golden, _ = matrix
    assert golden["fields"] == list(pkg.LAUNCH_FIELDS)
    assert golden["variants"] == [list(v) for v in lpc.VARIANTS]
    assert golden["skip_variants"] == [list(v) for v in lpc.SKIP_VARIANTS] and golden["skip_cases"] == list(lpc.SKIP_CASES)
    assert [c["name"] for c in cases] == list(golden["cases"])
    assert 200 <= len(cases) and set(lpc.SKIP_CASES) <= {c["name"] for c in cases}
    for c in cases:
        want = golden["cases"][c["name"]]
        if c["expect"] is None:
            assert [len(p) for p in want] == [len(lpc.variants(c))] * len(c["ch"]), c["name"]


def test_launch_plan_matches_parent(matrix):
    pkg, cases, golden, got_all = matrix
    wrong = []
    for case in cases:
        want, got = golden["cases"][case["name"]], got_all[case["name"]]
        if case["expect"] is not None:
            assert want == case["expect"] == got, case["name"]
            continue
        assert isinstance(got, list), (case["name"], got)
        for k, (gp, wp) in enumerate(zip(got, want)):
            for var, g, w in zip(lpc.variants(case), gp, wp):
                g, w = as_row(pkg, g), golden["rows"][w]
                if g != w:
                    nf = len(pkg.LAUNCH_FIELDS)
                    diff = [f for f, a, b in zip(pkg.LAUNCH_FIELDS, g, w) if a != b] + (["kernels"] if g[nf:] != w[nf:] else [])
                    wrong.append((case["name"], k, var, diff))
    assert not wrong, "%d launch plans differ from the recorded ones: %r" % (len(wrong), wrong[:20])


def test_the_two_cu_counts_take_both_paths(matrix):
    """what the 8-CU variants are in the matrix for"""
    pkg, cases, _, got = matrix
    one = got["geo-25M-1x16-f0-sw0"][0]  # one block of 2442 tiles
    assert one[0]["ev_chunk"] < one[2]["ev_chunk"]  # 256 CUs: the small-batch loop ran; 8: it did not
    big = got["big-2M6-400x16-f0-sw0-sk0"][0]
    assert big[2]["helpers"] == 16 and big[0]["helpers"] > 16  # 8 CUs: the cap wg_slots * oversub binds


def test_properties(matrix):
    pkg, cases, _, got_all = matrix
    model = (pkg.VARIANT_EV, pkg.VARIANT_EV_DENSE, pkg.VARIANT_PD_WIDE, pkg.VARIANT_PD_NARROW, pkg.VARIANT_EV_FIXED)
    synth_wg, ev_waves = 512, 16  # GPSBB_WG lanes, GPSBB_EV_WG / 64 wavefronts: the workgroups of k_synth and of the model kernels
    n = 0
    for case in cases:
        got = got_all[case["name"]]
        if not isinstance(got, list):
            continue
        for ch, per_variant in zip(case["ch"], got):
            nblocks, ntiles = ch.shape[0], (case["nsamp"] + 1023) // 1024
            for (cus, dg, skip), v in zip(lpc.variants(case), per_variant):
                where = (case["name"], cus, dg, skip)
                ids = [k[0] for k in v["kernels"]]
                synth = [k for k in v["kernels"] if k[0] % 256 >= pkg.LK_SYNTH0]
                # the variant and the kernel id agree, and so do the plan's geometry and the kernel's
                assert len(synth) == 1 and synth[0][0] % 256 == pkg.LK_SYNTH0 + v["variant"], where
                assert synth[0][0] // 256 == v["granule"] + 4 * v["digest_fused"], where
                assert synth[0][1:] == [v["grid_x"], v["grid_y"], v["wg"], v["lds"]], where
                assert v["last_kernel"] == (1 if v["variant"] == pkg.VARIANT_SYNTH else 2), where
                assert v["granule"] == 0 or v["variant"] == pkg.VARIANT_EV, where
                # fused digest implies no k_block_digest, and the reverse; none of either without a digest
                has_kbd = pkg.LK_BLOCK_DIGEST in ids
                assert has_kbd == (v["digest_gx"] > 0) and (has_kbd or v["digest_fused"]) == bool(dg), where
                assert not (has_kbd and v["digest_fused"]), where
                assert ids[-1] == (pkg.LK_BLOCK_DIGEST if has_kbd else synth[0][0]), where
                # the pre-pass resets the counters exactly for the lap-parallel and k_tiles forms
                fams = {i % 256 for i in ids}
                assert bool(v["ctr_reset"]) == (pkg.LK_LAP_PLAN in fams or pkg.LK_TILES in fams), where
                assert bool(v["ctr_reset"]) == (v["prepass"] in (pkg.PREPASS_LAPS, pkg.PREPASS_WALKS)), where
                if skip or v["prepass"] == pkg.PREPASS_HOST:
                    assert len(ids) == 1 + has_kbd and v["prepass"] == (pkg.PREPASS_SKIP if skip else pkg.PREPASS_HOST), where
                if v["prepass"] in (pkg.PREPASS_HOST, pkg.PREPASS_LAPS):
                    assert v["info_prepass"] == (2 if v["prepass"] == pkg.PREPASS_HOST else 3), where
                if v["variant"] in model:
                    # grid x = nblocks + helpers, and no helper that could not be useful
                    assert v["grid_x"] == nblocks + v["helpers"] and v["grid_y"] == 1, where
                    chunks = -(-ntiles // v["ev_chunk"])
                    max_useful = -(-chunks // ev_waves)
                    assert 0 <= v["helpers"] <= nblocks * (max_useful - 1), where
                    assert v["wg"] == 64 * ev_waves, where
                else:
                    assert v["helpers"] == 0 and v["grid_y"] == nblocks and v["wg"] == synth_wg, where
                n += 1
    assert n >= 4 * 500
