"""The fixed matrix of gpsbb_chain_carrier calls behind tests/test_chain_plan.py and tests/golden/chain_plans.json: every case is
one call, named, generated from numpy.random.default_rng(SEED).  cases() yields dicts:
  name, ch [nblocks, nch] descriptors, delt, nsamp, seed_where (the handle's GPSBB_OPT_SEED_WHERE), nblocks / nch (None, or the count
  to pass instead of the array's: the argument checks), limits: "default" or "lowered" (the process runs with LOWERED in its
  environment: the sub-batch limits are knobs of the experiments build, read once), expect: None or the error the call must return.

  python tests/chain_plan_cases.py FILE [lowered]    the cases of one limits group as tools/plan_asan.cpp reads them
  python tests/chain_plan_cases.py --plan GROUP      gpsbb_test_chain_plan over that group, as JSON {name: rc or values}
  python tests/chain_plan_cases.py --golden DEFAULT.txt LOWERED.txt   the record, from what the patched parent printed for the two
                                                     files (tools/experiments/chain_plan_dump_parent.patch)"""
import json
import sys

import numpy as np

import batch_plan_cases as bpc

SEED = 20261019
CHAIN = bpc.CHAIN
FS = 25e6
LOWERED = {"GPSBB_CHAIN_ONLY_BLOCKS": "16", "GPSBB_CHAIN_ONLY_LAPS": "2000"}
LIMITS = {"default": (16384, 6.0e6), "lowered": (16, 2000.0)}
EDGE_SHAPE, EDGE_NSAMP = (50, 5), 30000
E_BADARG, E_BADCHAN = -1, -2


def edges(ch):
    """What a sub-batch boundary can get wrong, on 50 blocks x 5 channels cut every 16 blocks (LOWERED)."""
    ch["prn"][16:, 0] = 21       # a PRN change exactly on a piece's first block
    ch["prn"][31:33, 1] = 0      # idle across the boundary at 32, back on the block after it
    ch["prn"][47, 4] = 0         # idle on a piece's last block, back on the next piece's first
    ch["f_carr"][:, 2] = 0.0     # a zero step: the phase stands still
    ch["f_carr"][:, 3] = -np.abs(ch["f_carr"][:, 3])  # a falling carrier
    return ch


def tiny(ch):
    ch["f_carr"][20, 4] = 1e-10  # one step with 0 < |f_carr * delt| < 2^-50: the row walks
    return ch


def edge_descriptors(pkg, with_tiny=False):
    """the boundary case, on its own generator: tests/test_chain_only_pieces_gpu.py runs the same descriptors on the device"""
    ch = edges(bpc.descriptors(np.random.default_rng(SEED + 1), pkg, *EDGE_SHAPE, False))
    return tiny(ch) if with_tiny else ch


def cases(pkg):
    rng = np.random.default_rng(SEED)
    out = []

    def add(name, ch, nsamp, limits="default", seed_where=0, expect=None, delt=1.0 / FS, nblocks=None, nch=None):
        out.append(dict(name=name, ch=ch, delt=delt, nsamp=nsamp, seed_where=seed_where, limits=limits, expect=expect,
                        nblocks=nblocks, nch=nch))

    # the lap limit at its default: 2.5 M samples of a 4 to 5 kHz carrier wrap 400 to 500 times, in lanes of 4 laps + 3: ~1 900 laps
    # per block of 16 channels, ~3 200 blocks per piece of 6.0e6 laps: 8 000 blocks cross the limit twice
    ch = bpc.descriptors(rng, pkg, 8000, 16, False)
    ch["f_carr"] = np.where(ch["f_carr"] < 0, -1.0, 1.0) * (4000.0 + 0.2 * np.abs(ch["f_carr"]))
    for sw in (0, 1):
        add("laps-8000x16-sw%d" % sw, ch, 2500000, seed_where=sw)
    # the block limit at its default: short blocks, few laps each
    ch = bpc.descriptors(rng, pkg, 16384 + 40, 5, False)
    for sw in (0, 1):
        add("blocks-16424x5-sw%d" % sw, ch, 30000, seed_where=sw)
    # lowered limits: the boundary descriptors, cut by the block limit on either path; a step only the row walks take; and longer
    # blocks (600 000 samples: ~65 laps per channel in lanes of one) that the lap limit cuts, every six blocks or so
    for sw in (0, 1):
        add("edges-50x5-sw%d" % sw, edge_descriptors(pkg), EDGE_NSAMP, "lowered", sw)
        add("edges-tiny-50x5-sw%d" % sw, edge_descriptors(pkg, True), EDGE_NSAMP, "lowered", sw)
        add("edges-long-50x5-sw%d" % sw, edge_descriptors(pkg), 600000, "lowered", sw)
    # errors, and what is none
    small = lambda: bpc.descriptors(rng, pkg, 3, 4, False)

    def edit(field, value, at=(1, 2)):
        ch = small()
        ch[field][at] = value
        return ch

    add("err-nch-0", small(), 30000, nch=0, expect=E_BADARG)
    add("err-nch-65", small(), 30000, nch=65, expect=E_BADARG)
    add("err-nsamp-0", small(), 0, expect=E_BADARG)
    add("err-delt-0", small(), 30000, delt=0.0, expect=E_BADARG)
    add("err-delt-inf", small(), 30000, delt=float("inf"), expect=E_BADARG)
    add("err-f-carr-nan", edit("f_carr", float("nan")), 30000, expect=E_BADCHAN)
    add("err-phase-minus-zero", edit("carr_phase", -0.0), 30000, expect=E_BADCHAN)
    add("err-phase-1p5", edit("carr_phase", 1.5), 30000, expect=E_BADCHAN)
    add("err-prn-33", edit("prn", 33), 30000, expect=E_BADCHAN)
    add("err-prn-minus-1", edit("prn", -1), 30000, expect=E_BADCHAN)
    over = 0.125 * FS  # the first f_carr whose product with delt, rounded as the library rounds it, exceeds an eighth
    while over * (1.0 / FS) <= 0.125:
        over = float(np.nextafter(over, np.inf))
    add("err-step-over-eighth", edit("f_carr", over), 30000, expect=E_BADCHAN)
    add("ok-step-eighth", edit("f_carr", -float(np.nextafter(over, 0.0))), 30000)
    ch = small()  # code fields the node driver never fills: not this call's business
    ch["f_code"], ch["code_phase"], ch["gain"], ch["iword"], ch["ibit"], ch["icode"] = float("nan"), -7.0, 1e300, -1, 99, 99
    add("ok-garbage-code-fields", ch, 30000)
    return out


def plan_group(pkg, group):
    """gpsbb_test_chain_plan over the cases of one limits group (the caller's environment holds the limits): {name: rc or values}"""
    got = {}
    for c in cases(pkg):
        if c["limits"] == group:
            rc, v = pkg.chain_plan(c["ch"], c["delt"], c["nsamp"], c["seed_where"], nblocks=c["nblocks"], nch=c["nch"])
            got[c["name"]] = rc if rc != 0 else v
    return got


def write_matrix(pkg, path, group):
    """One limits group as tools/plan_asan.cpp reads it (tests/batch_plan_cases.py, write_matrix: the same Record)."""
    rec = np.dtype([("nblocks", "<i4"), ("nch", "<i4"), ("nsamp", "<i4"), ("first", "<i4"), ("opt", "<i4", 5), ("carry", "<i4"),
                    ("fixed_prev", "<i4"), ("carry_prn", "<i4", 16), ("fx_prn", "<i4", 16), ("flags", "<u4"), ("fx_phase", "<u4", 16),
                    ("delt", "<f8")])
    with open(path, "wb") as f:
        for c in cases(pkg):
            if c["limits"] != group:
                continue
            nb = c["ch"].shape[0] if c["nblocks"] is None else c["nblocks"]
            nch = c["ch"].shape[1] if c["nch"] is None else c["nch"]
            ch = c["ch"] if (nb, nch) == c["ch"].shape else np.zeros((nb, nch), pkg.CHAN_DTYPE)
            r = np.zeros(1, rec)
            r["nblocks"], r["nch"], r["nsamp"], r["first"], r["flags"], r["delt"] = nb, nch, c["nsamp"], 1, CHAIN, c["delt"]
            r["opt"] = (c["seed_where"], 0, 0, 0, 6)
            f.write(r.tobytes())
            f.write(np.ascontiguousarray(ch).tobytes())


def golden_from_dumps(pkg, dumps):
    """tests/golden/chain_plans.json from the "chain ..." lines the patched parent printed for each group's file ({group: path})"""
    lines = {g: [l.split()[1:] for l in open(p) if l.startswith("chain ")] for g, p in dumps.items()}
    out = {}
    for c in cases(pkg):
        rc, *v = [int(x, 16) if k else int(x) for k, x in enumerate(lines[c["limits"]].pop(0))]
        out[c["name"]] = rc if rc != 0 else {"laps": v[0], "npieces": v[1], "h_cd": v[2], "h_start0": v[3],
                                             "pieces": [v[4 + 4 * k:8 + 4 * k] for k in range(v[1])]}
    assert not any(lines.values())
    return {"cases": out}


if __name__ == "__main__":
    from conftest import load_package
    if sys.argv[1] == "--plan":
        print(json.dumps(plan_group(load_package(), sys.argv[2])))
    elif sys.argv[1] == "--golden":
        print(json.dumps(golden_from_dumps(load_package(), {"default": sys.argv[2], "lowered": sys.argv[3]}), indent=1))
    else:
        write_matrix(load_package(), sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "default")
