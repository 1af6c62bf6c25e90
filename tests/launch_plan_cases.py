"""The matrix behind tests/test_launch_plan.py and tests/golden/launch_plans.json: every set-up of tests/batch_plan_cases.py (a ring's
pushes each on their own), taken at two CU counts, without and with the blocks' digests; a few of them also as a run that
GPSBB_OPT_SKIP_SEED leaves without its pre-pass.

    python tests/launch_plan_cases.py DUMP tests/golden/launch_plans.json

turns the lines tools/launch_dump.cpp printed (tools/experiments/launch_dump_parent.patch: the commit before plan_launch existed, its
launch path run on a CPU) over the matrix `python tests/batch_plan_cases.py FILE` wrote into the record: the distinct lines once
("rows": the LAUNCH_FIELDS, the number of kernels, five numbers per kernel), and per case and push the row of every variant."""
import json

import batch_plan_cases as bpc

# 256: an MI355X.  8: few enough that the helpers of a 400-block batch stop at wg_slots * oversub = 16, and that a single block of 2442
# tiles keeps its chunks of four (at 256 CUs the small-batch loop takes them down to one)
CUS = (256, 8)
VARIANTS = [(cus, dg, 0) for cus in CUS for dg in (0, 1)]  # (CUs, want_digest, skip)
SKIP_VARIANTS = [(256, 0, 1), (8, 1, 1)]
# one per pre-pass kind: lap-parallel, row walks with the chain, k_seed behind a start-phase chain, host threads, a ring's push
SKIP_CASES = ("geo-25M-4x16-f1-sw0", "geo-2M6-5x16-f1-sw1", "geo-1M-5x16-f1-sw1", "opt-4x16-f0-sw2-sk0", "ring-carry-5x16-sw0-sk0")
DUMP_ORDER = [(cus, dg, skip) for cus in CUS for dg in (0, 1) for skip in (0, 1)]  # tools/launch_dump.cpp's loops


def variants(case):
    return VARIANTS + (SKIP_VARIANTS if case["name"] in SKIP_CASES else [])


def record(pkg, dump_path):
    rows, index, out = [], {}, {}
    with open(dump_path) as f:
        lines = [[int(x) for x in l.split()] for l in f]
    at = 0
    for case in bpc.cases(pkg):
        pushes = []
        for _ in case["ch"]:
            got = dict(zip(DUMP_ORDER, lines[at:at + len(DUMP_ORDER)]))
            at += len(DUMP_ORDER)
            if got[DUMP_ORDER[0]][0] != 0:
                pushes = got[DUMP_ORDER[0]][0]  # the error set-up returns
                break
            pushes.append([index.setdefault(tuple(got[v][1:]), len(index)) for v in variants(case)])
        out[case["name"]] = pushes
    assert at == len(lines), (at, len(lines))
    rows = [list(r) for r, _ in sorted(index.items(), key=lambda kv: kv[1])]
    return {"fields": list(pkg.LAUNCH_FIELDS), "variants": VARIANTS, "skip_variants": SKIP_VARIANTS, "skip_cases": list(SKIP_CASES),
            "rows": rows, "cases": out}


if __name__ == "__main__":
    import sys
    from conftest import load_package
    with open(sys.argv[2], "w") as f:
        json.dump(record(load_package(), sys.argv[1]), f, separators=(",", ":"))
        f.write("\n")
