"""The chip table of the model kernels (EvLdsT::chip2, pluto-gps-sim_amd/csrc/gpsbb_events.hip.h): the low byte of an entry is the
sign of chip c, the high byte a flag — 0x0f where chip c + 1 has the same sign, 0 where it differs — which ev_second ORs into the
chip change's row: equal neighbours send the change to the discard row, and the sign behind the change is simply the inverse of
the sign before it.  The cases put chip boundaries of both kinds on the first, the last and a middle sample of lane runs, take the
code through chips 1022 -> 1023 -> 0 with and without a data-bit change (the entries at and past 1022; the instances that still
compare chip indices), send lanes to the exact path, and render the same blocks through every instance that shares the code:
k_synth_ev, k_synth_ev_digest, k_synth_ev_fixed, k_synth_ev_dense.

Everything is 16 channels at 25 MS/s, three blocks of 2 * 1024 + 40 samples (the `exact` case: the prologue test's), bit for bit
against the CPU oracle (IQ and end states).  Every case also asserts GPSBB_INFO_LAST_VARIANT, that the hazard counters are the
oracle's, and that the exact-run and hazard counters are those the kernels gave for the same input BEFORE the table changed
(PARENT below: positions and tests are the same, so the same lanes take the exact path).

PARENT was measured on an MI355X with the parent commit's library
(`GPSBB_PY_LIB=<the parent's libgpsbb.so> python tools/cf01_counters.py`)."""
import numpy as np
import pytest

import contract_corners as cc
import test_ev_tile_prologue_gpu as tp

pytestmark = pytest.mark.gpu

FS = 25e6
DELT = 1.0 / FS
TILE = 1024
SPT = 16                      # samples of a lane's run
NB, NCH, NSAMP = 3, 16, 2 * TILE + 40
CA_LEN = 1023

# exact-run and hazard counters of the parent commit's kernels (case, instance -> exact runs, itable_512, dwrd_oob)
PARENT = {
    "neighbours ev": (0, 0, 0),
    "neighbours digest": (0, 0, 0),
    "neighbours fixed": (0, 0, 0),
    "neighbours dense": (0, 0, 0),
    "wrap-mid ev": (0, 0, 0),
    "wrap-last-run ev": (204, 0, 0),   # the four channels at 0.064 chips per sample: 15.5 steps are 0.992 chips, the bias W is wide
    "databit ev": (0, 0, 0),
    "databit digest": (0, 0, 0),
    "databit fixed": (0, 0, 0),
    "databit dense": (0, 0, 0),
    "exact ev": (2, 0, 0),
}

# f_carr of the per-sample class at 25 MS/s: 4.8 table-index changes in a run of 15.5 samples, more than the breakpoint path takes
F_CARR_DENSE = 0.3 / 15.5 / 512 * FS * 16


def descriptors(pkg, seed):
    ch = pkg.synth_descriptors(NB, nch=NCH, seed=seed)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    return ch


def chips(pkg, prn):
    """the PRN's 1023 chips, and whether chip c and chip c + 1 (chip 1023 is chip 0) are equal"""
    ca = np.asarray(pkg.codegen(int(prn))).astype(np.int64)
    return ca, ca == np.roll(ca, -1)


def crossed(ch, nsamp):
    """[block, channel] -> (chips c whose boundary to c + 1 the block crosses, not reduced modulo 1023)"""
    sc = ch["f_code"] * DELT
    lo = np.floor(ch["code_phase"]).astype(np.int64)
    hi = np.floor(ch["code_phase"] + sc * (nsamp - 1)).astype(np.int64)
    return lo, hi


# ---- neighbours -----------------------------------------------------------------------------------------------------------
# where in a lane's run the placed boundary falls: the new chip's first sample is the run's first, its last, one in the middle
RUN_AT = (0, SPT - 1, 7)


def neighbours_case(pkg):
    """channel i: a chip boundary whose first sample behind it is sample RUN_AT[i % 3] of lane 3 + 2 i's run of tile i % 2, between
    equal neighbours for (i // 3) even and differing ones for odd; no roll-over in the block"""
    ch = descriptors(pkg, 0xCF01)
    sc = ch["f_code"] * DELT
    placed = np.zeros((NB, NCH), np.int64)
    for b in range(NB):
        for i in range(NCH):
            _, eq = chips(pkg, ch["prn"][b, i])
            want_equal = (i // 3) % 2 == 0
            c = next(c for c in range(200 + 40 * b + 7 * i, 900) if bool(eq[c]) == want_equal)  # the boundary between chips c and c + 1
            n = (i % 2) * TILE + (3 + 2 * i) * SPT + RUN_AT[i % 3]   # the first sample on chip c + 1
            ch["code_phase"][b, i] = (c + 1) - sc[b, i] * (n - 0.5)
            placed[b, i] = c
    ch["icode"] = 4
    # what the placements are for: the boundary is where it was put, and every channel crosses boundaries of both kinds
    x = ch["code_phase"]
    lo, hi = crossed(ch, NSAMP)
    assert (lo >= 0).all() and (hi < CA_LEN).all()
    for b in range(NB):
        for i in range(NCH):
            n = (i % 2) * TILE + (3 + 2 * i) * SPT + RUN_AT[i % 3]
            assert int(np.floor(x[b, i] + sc[b, i] * (n - 1))) == placed[b, i] and int(np.floor(x[b, i] + sc[b, i] * n)) == placed[b, i] + 1
            _, eq = chips(pkg, ch["prn"][b, i])
            kinds = eq[lo[b, i]:hi[b, i]]
            assert kinds.any() and not kinds.all(), (b, i)
    return ch, NSAMP, pkg.CHAIN_CARRIER


# ---- wrap -----------------------------------------------------------------------------------------------------------------

def wrap_case(pkg, last_run):
    """chips 1022 -> 1023 -> 0 and the same data bit behind the roll-over.  last_run: the roll-over in the last run of tile 0, at
    each of its 16 samples — the anchor of tile 1 of the granule then lies in [1023, 1024), is not reduced, and the tile's chip
    index goes on past 1023 for all of its 1024 samples; four channels at a code step of 0.064 chips per sample (the fastest the
    breakpoint kernels take is 1 / 15.5) reach index 1089 of the table's 1104 entries.  Otherwise: in the middle of tiles 0, 1, 2."""
    ch = descriptors(pkg, 0xCF02 + int(last_run))
    if last_run:
        ch["f_code"][:, 12:] = 0.064 * FS
    sc = ch["f_code"] * DELT
    for i in range(NCH):
        at = (TILE - SPT + i) if last_run else (150 + 61 * i, TILE + 90 + 53 * i, 2 * TILE + i // 3 + 1)[i % 3]
        ch["code_phase"][:, i] = CA_LEN - sc[:, i] * (at + 0.5)   # chip 1023 is reached between samples `at` and `at` + 1
    ch["icode"] = 4
    x = ch["code_phase"]
    lo, hi = crossed(ch, NSAMP)
    assert (lo <= 1021).all() and (hi >= 1024).all()  # chips 1022, 1023 (= 0) and 1024 (= 1) are all rendered
    if last_run:
        anchor1 = x + TILE * sc                       # the model's anchor of tile 1: the block's start phase 1024 steps on
        assert ((anchor1 >= CA_LEN) & (anchor1 < CA_LEN + 1)).all()
        assert (np.floor(anchor1 + (TILE - 1) * sc)[:, 12:] >= 1088).all()
    return ch, NSAMP, pkg.CHAIN_CARRIER


# ---- databit --------------------------------------------------------------------------------------------------------------
# the sample before the roll-over (chip 1023 is reached between samples `at` and `at` + 1), per channel: the roll-over inside a
# run whose first sample is on chip 1022 (at = 16 l + 7, + 14: the change on the run's last sample; 16 l: on its second), a run
# whose first sample is the first on chip 1023 (at = 16 l - 1), tiles 0, 1 and the partial tile 2, and the prologue test's anchors
ROLL_AT = (5 * SPT + 7, 9 * SPT - 1, 12 * SPT + 14, TILE + 3 * SPT, TILE + 20 * SPT + 7, 40 * SPT - 1, 1014, TILE + 47 * SPT - 1,
           2 * TILE + SPT - 1, 2 * TILE + 7, 500, 1023, 33 * SPT + 14, TILE + 9 * SPT - 1, TILE + 300, 61 * SPT)
F_CARR_KC = (1200.0, 4900.0, -4900.0)   # one table-index change per run at most; two, rising and falling


def databit_case(pkg):
    ch = descriptors(pkg, 0xCF04)
    for i in range(NCH):
        ch["f_carr"][:, i] = F_CARR_KC[i % 3]
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    sc = ch["f_code"] * DELT
    for i in range(NCH):
        ch["code_phase"][:, i] = CA_LEN - sc[:, i] * (ROLL_AT[i] + 0.5)
        if i < 12:
            ch["icode"][:, i] = 19                                # the roll-over ends a data bit ...
            ch["dwrd"][:, i, :] = 0x2AAAAAAA if i % 2 == 0 else 0x15555555  # ... and the next one differs (alternating words)
            ch["ibit"][:, i] = 3 + i
        else:
            ch["icode"][:, i] = 4                                 # the same data bit goes on behind the roll-over
    # what the placements are for: in every channel some lane's first sample sits on chip 1022 and some lane's on chip 1023
    n = np.arange(0, NSAMP, SPT)
    x = ch["code_phase"]
    first = np.floor(x[0][:, None] + sc[0][:, None] * n[None, :]).astype(np.int64)   # [channel, lane run]: as the model, not reduced
    assert (first == 1022).any(axis=1).all() and (first == 1023).any(axis=1).all()
    return ch, NSAMP, pkg.CHAIN_CARRIER


def exact_case(pkg):
    return tp.carrier_case(pkg, 16)


CASES = {
    "neighbours": neighbours_case,
    "wrap-mid": lambda pkg: wrap_case(pkg, False),
    "wrap-last-run": lambda pkg: wrap_case(pkg, True),
    "databit": databit_case,
    "exact": exact_case,
}


def instance_of(pkg, case, inst):
    """the case's descriptors for one instance of the shared code -> ch, nsamp, batch flags, oracle keywords, GPSBB_VARIANT_*"""
    ch, nsamp, flags = CASES[case](pkg)
    if inst == "fixed":      # k_synth_ev_fixed: the 32-bit carrier accumulator
        return cc.fixed_of(ch), nsamp, flags | pkg.FIXED_CARRIER, dict(chain=True, fixed=True), pkg.VARIANT_EV_FIXED
    if inst == "dense":      # k_synth_ev_dense: channel 15's carrier is evaluated per sample, the others by breakpoints
        ch = ch.copy()
        ch["f_carr"][:, 15] = F_CARR_DENSE
        return ch, nsamp, flags, dict(chain=True), pkg.VARIANT_EV_DENSE
    return ch, nsamp, flags, dict(chain=True), pkg.VARIANT_EV   # "ev", "digest": k_synth_ev, k_synth_ev_digest


_wanted = {}


def wanted(pkg, oracle, case, inst):
    """the oracle's rendering, once per (case, descriptors): "ev" and "digest" share theirs"""
    key = (case, "ev" if inst == "digest" else inst)
    if key not in _wanted:
        ch, nsamp, _, kw, _ = instance_of(pkg, case, inst)
        iq, st, hz = oracle.fill_blocks(ch, DELT, nsamp, **kw)
        iq.setflags(write=False)
        _wanted[key] = (iq, st, hz)
    return _wanted[key]


def render(pkg, synth, case, inst):
    """-> IQ, end states, the counters' growth (exact runs, itable_512, dwrd_oob, tiles), GPSBB_INFO_LAST_VARIANT, and for the
    digest instance the popped digests"""
    ch, nsamp, flags, _, _ = instance_of(pkg, case, inst)
    c0 = tp.counters(pkg, synth)
    dig = None
    if inst == "digest":
        q = synth.stream(NCH, DELT, nsamp, ch.shape[0], depth=2, flags=flags | pkg.STREAM_DEVICE_ONLY)
        q.push(ch, digest=True)
        synth.sync()
        got = tp.counted(pkg, synth, c0)
        variant = synth.info(pkg.INFO_LAST_VARIANT)
        ptr, st, dig = q.pop_digest()
        iq = synth.device_read(ptr, (ch.shape[0], nsamp, 2))
        q.close()
    else:
        b = synth.batch(ch, DELT, nsamp, flags=flags)
        b.run(); synth.sync()
        got = tp.counted(pkg, synth, c0)
        variant = synth.info(pkg.INFO_LAST_VARIANT)
        iq, st = b.read()
        b.close()
    return iq, st, got, variant, dig


def check(pkg, synth, oracle, case, inst):
    name = "%s %s" % (case, inst)
    ch, nsamp, _, _, variant = instance_of(pkg, case, inst)
    want_iq, want_st, hz = wanted(pkg, oracle, case, inst)
    iq, st, got, got_variant, dig = render(pkg, synth, case, inst)
    print("%s: exact runs %d, itable_512 %d, dwrd_oob %d, tiles %d" % ((name,) + got))
    assert got_variant == variant and synth.info(pkg.INFO_LAST_KERNEL) == 2, (name, got_variant)
    assert got[3] == ch.shape[0] * ((nsamp + TILE - 1) // TILE), (name, got)
    bad = np.nonzero((iq != want_iq).any(axis=(1, 2)))[0]
    assert bad.size == 0, (name, "blocks whose IQ differs", bad.tolist(), "first sample", int(np.nonzero((iq[bad[0]] != want_iq[bad[0]]).any(axis=1))[0][0]))
    assert tp.same_states(st, want_st, ch) == [], name
    if dig is not None:
        assert (dig == pkg.block_digest_host(want_iq)).all(), name
    assert (got[1], got[2]) == (int(hz["itable_512"]), int(hz["dwrd_oob"])), (name, got, hz)
    assert got[:3] == tuple(PARENT[name]), (name, got, PARENT[name])


@pytest.fixture()
def fresh(pkg, synth):
    for opt in (pkg.OPT_SEED_WHERE, pkg.OPT_SYNTH_KERNEL, pkg.OPT_CHAIN_WHERE):
        synth.set_option(opt, 0)
    yield synth


def test_neighbours(pkg, fresh, oracle):
    """chip boundaries between equal and between differing neighbours on the first, the last and a middle sample of lane runs"""
    check(pkg, fresh, oracle, "neighbours", "ev")


@pytest.mark.parametrize("where", ["mid", "last-run"])
def test_wrap(pkg, fresh, oracle, where):
    """chips 1022 -> 1023 -> 0 inside a tile with the data bit going on: the table's entries at and past 1022, up to its top"""
    check(pkg, fresh, oracle, "wrap-" + where, "ev")


def test_databit(pkg, fresh, oracle):
    """the roll-over ends a data bit and the next one differs: the instances that compare the chip index with 1023 and 1022, for
    channels with one and with two table-index changes per run"""
    check(pkg, fresh, oracle, "databit", "ev")


def test_exact(pkg, fresh, oracle):
    """the prologue test's carriers-16 descriptors: lanes on the exact path, as many as before the table changed"""
    check(pkg, fresh, oracle, "exact", "ev")
    assert PARENT["exact ev"][0] > 0


@pytest.mark.parametrize("inst", ["digest", "fixed", "dense"])
@pytest.mark.parametrize("case", ["neighbours", "databit"])
def test_the_other_instances(pkg, fresh, oracle, case, inst):
    """the same blocks through k_synth_ev_digest (GPSBB_PUSH_DIGEST, a device-only ring), k_synth_ev_fixed (GPSBB_FIXED_CARRIER)
    and k_synth_ev_dense (one channel's carrier in the per-sample class)"""
    check(pkg, fresh, oracle, case, inst)
