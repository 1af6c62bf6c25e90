"""plan_push_side (csrc/gpsbb_plan.h): on which side a ring's push chains its IEEE carrier — not at all (the ring is not chained,
or chains the accumulator), on host threads, or on the device — through gpsbb_test_push_side, against the table below.  No GPU:
the side is plain arithmetic on the descriptors and the options, the same function gpsbb_stream_push asks.

The rule the table spells out: GPSBB_OPT_CHAIN_WHERE 1 and GPSBB_OPT_SEED_WHERE 2 mean the host; seed_where 1 and 3 mean the
device; left to the library (0), a push of more than HOST_SEED_MAX_CHANNELS = 64 block-channels goes to the device, and a smaller
one only where the lap-parallel pre-pass will take it: no option that keeps the laps away (the per-sample kernel, chain_where 2
or 3), no carrier step below 2^-50, a rate the model kernels render.

And what ties the side to the rest of the plan: a DEVICE push is planned with the stream's carry, and plan_batch then resolves
the chain on the device and never seeds on the host; a HOST push is planned without GPSBB_CHAIN_CARRIER (gpsbb_stream_push has
resolved the chain into the descriptors), and plan_batch then runs no chain across blocks on the device."""
import numpy as np
import pytest

import batch_plan_cases as bpc
from conftest import load_package

CHAIN, FIXED = bpc.CHAIN, bpc.FIXED
NONE, HOST, DEVICE = 0, 1, 2
SMALL = (25e6, 4096)  # with 2 x 4 channels: the small push the laps keep on the device
E_BADCHAN = -2


def tiny(ch):
    ch["f_carr"][:, 2] = 1e-10  # |f_carr * delt| < 2^-50 at either rate: the laps decline
    return ch


def bad_prn(ch):
    ch["prn"][1, 3] = 33
    return ch


# name, (nblocks, nch), geometry, flags, options, edit of the descriptors, the side (or the error)
ROWS = [
    ("small", (2, 4), SMALL, CHAIN, {}, None, DEVICE),
    ("small-per-sample", (2, 4), SMALL, CHAIN, dict(synth_kernel=1), None, HOST),
    ("small-cw2", (2, 4), SMALL, CHAIN, dict(chain_where=2), None, HOST),
    ("small-cw3", (2, 4), SMALL, CHAIN, dict(chain_where=3), None, HOST),
    ("small-tiny", (2, 4), SMALL, CHAIN, {}, tiny, HOST),
    ("small-1M", (2, 4), "1M", CHAIN, {}, None, HOST),  # the model kernels decline 1 MS/s
    ("64-per-sample", (4, 16), "2M6", CHAIN, dict(synth_kernel=1), None, HOST),
    ("80-per-sample", (5, 16), "2M6", CHAIN, dict(synth_kernel=1), None, DEVICE),
    ("64-default", (4, 16), "2M6", CHAIN, {}, None, DEVICE),  # by the laps
    ("64-tiny", (4, 16), "2M6", CHAIN, {}, tiny, HOST),
    ("80-tiny", (5, 16), "2M6", CHAIN, {}, tiny, DEVICE),  # by size: the row walks
    ("small-plain", (2, 4), SMALL, 0, {}, None, NONE),
    ("small-fixed", (2, 4), SMALL, FIXED, {}, None, NONE),
    ("small-fixed-chain", (2, 4), SMALL, FIXED | CHAIN, {}, None, NONE),
    ("80-plain", (5, 16), "2M6", 0, dict(seed_where=1), None, NONE),
    ("80-fixed", (5, 16), "2M6", FIXED, dict(seed_where=1), None, NONE),
    ("80-fixed-chain", (5, 16), "2M6", FIXED | CHAIN, dict(seed_where=1), None, NONE),
    ("small-bad-prn", (2, 4), SMALL, CHAIN, {}, bad_prn, E_BADCHAN),
    ("80-bad-prn-host", (5, 16), "2M6", CHAIN, dict(seed_where=2), bad_prn, E_BADCHAN),
]
# every GPSBB_OPT_SEED_WHERE x GPSBB_OPT_CHAIN_WHERE on 5 x 16:   chain_where 0     1     2       3
OPTIONS_5x16 = {0: (DEVICE, HOST, DEVICE, DEVICE),
                1: (DEVICE, HOST, DEVICE, DEVICE),
                2: (HOST, HOST, HOST, HOST),
                3: (DEVICE, HOST, DEVICE, DEVICE)}
ROWS += [("80-sw%d-cw%d" % (sw, cw), (5, 16), "2M6", CHAIN, dict(seed_where=sw, chain_where=cw), None, OPTIONS_5x16[sw][cw])
         for sw in range(4) for cw in range(4)]


@pytest.fixture(scope="module")
def sides():
    """every row once: (row, descriptors, delt, nsamp, rc, side)"""
    pkg = load_package()
    pkg.build()
    rng = np.random.default_rng(bpc.SEED)
    out = []
    for row in ROWS:
        name, (nblocks, nch), geo, flags, opts, edit, want = row
        fs, nsamp = bpc.GEOMETRIES[geo] if isinstance(geo, str) else geo
        ch = bpc.descriptors(rng, pkg, nblocks, nch, bool(flags & FIXED))
        if edit:
            ch = edit(ch)
        rc, side = pkg.push_side(ch, 1.0 / fs, nsamp, flags, **opts)
        out.append((row, ch, 1.0 / fs, nsamp, rc, side))
    return pkg, out


def test_side_matches_the_table(sides):
    _, rows = sides
    assert {DEVICE, HOST, NONE, E_BADCHAN} == {row[-1] for row, *_ in rows}
    wrong = [(row[0], rc, side, row[-1]) for row, _, _, _, rc, side in rows if (rc if rc else side["chain"]) != row[-1]]
    assert not wrong, "(row, rc, side, wanted): %r" % wrong


def test_first_plan_step_is_handed_on_only_where_it_was_needed(sides):
    """plan_begin runs inside the decision only for a small push the options leave to the laps; every other row's plan starts in
    batch set-up"""
    _, rows = sides
    for row, ch, _, _, rc, side in rows:
        if rc:
            continue
        asked = row[3] == CHAIN and ch.size <= 64 and not any(row[4].values()) and row[5] is not tiny
        assert side["begun"] == int(asked), row[0]


def test_device_side_is_planned_as_a_device_side_chain(sides):
    pkg, rows = sides
    n = 0
    for row, ch, delt, nsamp, rc, side in rows:
        if rc or side["chain"] != DEVICE:
            continue
        rc, v = pkg.plan(ch, delt, nsamp, row[3], max_sets=1, carry_prn=np.zeros(pkg.MAX_CHAN, np.int32),
                         carry_phase=np.zeros(pkg.MAX_CHAN, np.float64), **row[4])
        assert rc == 0 and v["chain_dev"] == 1 and v["host_seed"] == 0, row[0]
        n += 1
    assert n >= 12


def test_host_side_is_planned_without_a_chain_across_blocks(sides):
    pkg, rows = sides
    n = 0
    for row, ch, delt, nsamp, rc, side in rows:
        if rc or side["chain"] != HOST:
            continue
        rc, v = pkg.plan(ch, delt, nsamp, row[3] & ~CHAIN, max_sets=1, **row[4])
        assert rc == 0 and (v["chain_dev"] == 0 or v["chain_indep"] == 1), row[0]
        n += 1
    assert n >= 12
