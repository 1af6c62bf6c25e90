"""The data bits of a granule table travel in the signs of its code states (ev_nav_in_sign,
pluto-gps-sim_amd/csrc/gpsbb_events.hip.h): k_lap_pass2<., ., 1> sets the sign where the data bit in force at a granule's first
sample is -1 and writes no tile_nav word, k_synth_ev<1> / k_synth_ev_digest<1> take the magnitude and get the bit in force from
the sign of the granule's state and the bit after the granule's roll-over from the sign of the row's next state — behind the row's
last state from the dataBit of the block's end state.

16 channels at 25 MS/s, blocks of 3 to 5 code periods (75 000, 77 824, 100 352 and 125 000 samples: a partial last tile that is
tile 1 of the last granule, whole granules, and a partial last tile that is tile 0 of a one-tile last granule), bit for bit
against the CPU oracle: IQ and end states.  The descriptors put the roll-over that ends a data bit (the next bit differs) between
samples E and E + 1 of a block, per channel (EDGES): in tile 0 and in tile 1 of a granule, on the last sample of either, in the
block's last granule, in its partial last tile, on its last step, on channels with a falling carrier (rendered mirrored), and on
one channel of a pair while the other has no edge in the whole block.  A code period is 25 000 samples, so an edge E samples into a
block is the block's (E // 25 000 + 1)-th roll-over and icode starts at 19 - E // 25 000: 19 and 18 for the edges of the first two
periods, lower for the edges that must lie at a block's end.  Two more cases: every data bit -1 from the first sample to the
last (the sign is set on every state; channel 0 starts at code phase 0.0, stored as -0.0), and every channel starting at exactly
0.0 with alternating bits.

Every case goes once through a CHAIN_CARRIER | STREAM_DEVICE_ONLY ring of two pushes (k_synth_ev<1>), once in one push with
GPSBB_PUSH_DIGEST (k_synth_ev_digest<1>), and once through the per-sample kernel (GPSBB_OPT_SYNTH_KERNEL 1), whose tables keep
tile_nav.  The exact-run and hazard counters must be the oracle's and those of the parent commit's kernels for the same input
(PARENT: measured on an MI355X with the parent's library, `GPSBB_PY_LIB=<its libgpsbb.so> python tools/nv01_counters.py`, commit
a39915f): the model and its tests have not moved, so the same lanes take the exact path."""
import numpy as np
import pytest

import test_ev_tile_prologue_gpu as tp

pytestmark = pytest.mark.gpu

FS = 25e6
DELT = 1.0 / FS
TILE = 1024
GRAN = 2 * TILE               # samples of a code granule (GPSBB_EV_STATE_LOG2 = 1)
NCH, BPS = 16, 2              # channels; blocks per push (a ring of two pushes renders 2 * BPS blocks)
CA_LEN = 1023
F_CARR = (1200.0, 4900.0, -4900.0, -1200.0)   # one table-index change per run at most, two; rising and falling

# exact-run and hazard counters of the parent commit's kernels: "case run" -> (exact runs, itable_512, dwrd_oob)
PARENT = {
    "edges-75000 ring": (0, 0, 0), "edges-75000 digest": (0, 0, 0), "edges-75000 per-sample": (0, 0, 0),
    "edges-125000 ring": (0, 0, 0), "edges-125000 digest": (0, 0, 0), "edges-125000 per-sample": (0, 0, 0),
    "minus ring": (4, 0, 0), "minus digest": (4, 0, 0), "minus per-sample": (0, 0, 0),
    "zero ring": (64, 0, 0), "zero digest": (64, 0, 0), "zero per-sample": (0, 0, 0),   # a phase of exactly 0.0: the low word is 0
}


def edges_of(nsamp):
    """channel -> E: the roll-over that ends the data bit falls between samples E and E + 1 (None: no edge in the block)"""
    ntiles = (nsamp + TILE - 1) // TILE
    last_tile = (ntiles - 1) * TILE                 # the partial last tile's first sample
    last_gran = ((ntiles - 1) // 2) * GRAN          # the last granule's
    e = [10 * GRAN + 300,                           # 0: tile 0 of a granule ...
         None,                                      # 1: ... and its neighbour in the channel order has none
         10 * GRAN + TILE + 300,                    # 2: tile 1 of a granule
         last_gran + 37,                            # 3: the block's last granule (the bit behind it: the end state's)
         last_tile + (nsamp - last_tile) // 2,      # 4: the block's partial last tile
         7 * GRAN + 611,                            # 5: tile 0, falling carrier (F_CARR[5 % 4] < 0)
         21 * GRAN + TILE + 77,                     # 6: tile 1, falling carrier (the fast one)
         12 * GRAN - 1,                             # 7: the new bit's first sample is a granule's first
         12 * GRAN + TILE - 1,                      # 8: ... is tile 1's first
         nsamp - 1,                                 # 9: on the block's last step: only the end state sees the new bit
         5,                                         # 10: the block's first run
         last_gran - 1,                             # 11: the new bit's first sample is the last granule's first
         None,                                      # 12
         30 * GRAN + 2 * 16 + 15,                   # 13: the last sample of a lane's run
         30 * GRAN + TILE + 5 * 16,                 # 14: the first sample of a lane's run
         nsamp - 2]                                 # 15: the new bit holds for the block's last sample alone
    assert all(x is None or 0 <= x < nsamp for x in e)
    return e


def base(pkg, nblocks, seed):
    ch = pkg.synth_descriptors(nblocks, nch=NCH, seed=seed)
    for i in range(NCH):
        ch["f_carr"][:, i] = F_CARR[i % 4] * (1.0 + 0.01 * i)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    ch["iword"] = 2
    ch["ibit"] = 3 + np.arange(NCH)[None, :]
    return ch


def edges_case(pkg, nsamp):
    ch = base(pkg, 2 * BPS, 0x4E01 + nsamp)
    sc = ch["f_code"] * DELT
    for b in range(2 * BPS):
        for i, E in enumerate(edges_of(nsamp)):
            if E is None:
                ch["dwrd"][b, i, :] = 0x3FFFFFFF if (b + i) % 2 else 0      # one bit, + or -, for good
                ch["icode"][b, i] = 7
                continue
            E = min(E + 3 * b, nsamp - 1) if E < nsamp - 2 else E           # (not the same sample in every block)
            adv = sc[b, i] * (E + 0.5)
            m = int(adv // CA_LEN) + 1                                       # it is the block's m-th roll-over
            ch["code_phase"][b, i] = m * CA_LEN - adv
            ch["icode"][b, i] = 20 - m
            ch["dwrd"][b, i, :] = 0x2AAAAAAA if (b + i) % 2 else 0x15555555  # alternating bits: the next one differs
    assert (ch["code_phase"] >= 0).all() and (ch["code_phase"] < CA_LEN).all() and (ch["icode"] >= 0).all() and (ch["icode"] < 20).all()
    return ch, nsamp


def minus_case(pkg):
    """every data bit -1: the sign is set on every code state of the tables; channel 0 starts at 0.0"""
    ch = base(pkg, 2 * BPS, 0x4E02)
    ch["dwrd"] = 0
    ch["icode"] = 18
    ch["code_phase"][:, 0] = 0.0
    return ch, 49 * GRAN


def zero_case(pkg):
    """every channel starts a block at a code phase of exactly 0.0; alternating bits from icode 19 and 18: edges 25 000 k samples on"""
    ch = base(pkg, 2 * BPS, 0x4E03)
    ch["code_phase"] = 0.0
    ch["icode"] = np.where(np.arange(NCH) % 2, 19, 18)[None, :]
    ch["dwrd"] = np.where(np.arange(NCH) % 4 < 2, 0x2AAAAAAA, 0x15555555).astype(np.uint32)[None, :, None]
    return ch, 38 * GRAN


CASES = {
    "edges-75000": lambda pkg: edges_case(pkg, 75000),
    "edges-125000": lambda pkg: edges_case(pkg, 125000),
    "minus": minus_case,
    "zero": zero_case,
}
RUNS = ("ring", "digest", "per-sample")

_wanted = {}


def wanted(pkg, oracle, case):
    """the oracle's rendering of the case's 2 * BPS chained blocks, once"""
    if case not in _wanted:
        ch, nsamp = CASES[case](pkg)
        iq, st, hz = oracle.fill_blocks(ch, DELT, nsamp, chain=True)
        iq.setflags(write=False)
        _wanted[case] = (ch, nsamp, iq, st, hz)
    return _wanted[case]


def render(pkg, synth, ch, nsamp, run):
    """-> IQ, end states, the counters' growth (exact runs, itable_512, dwrd_oob, tiles), the digests (run "digest")"""
    flags = pkg.CHAIN_CARRIER
    nb = ch.shape[0]
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 1 if run == "per-sample" else 0)
    c0 = tp.counters(pkg, synth)
    dig = None
    if run == "per-sample":
        b = synth.batch(ch, DELT, nsamp, flags=flags)
        b.run(); synth.sync()
        got = tp.counted(pkg, synth, c0)
        assert synth.info(pkg.INFO_LAST_KERNEL) == 1
        iq, st = b.read()
        b.close()
        return iq, st, got, dig
    per = nb if run == "digest" else BPS
    q = synth.stream(NCH, DELT, nsamp, per, depth=2, flags=flags | pkg.STREAM_DEVICE_ONLY)
    iqs, sts, digs = [], [], []
    for lo in range(0, nb, per):
        q.push(ch[lo:lo + per], digest=(run == "digest"))
    synth.sync()
    got = tp.counted(pkg, synth, c0)
    assert synth.info(pkg.INFO_LAST_KERNEL) == 2 and synth.info(pkg.INFO_LAST_VARIANT) == pkg.VARIANT_EV and synth.info(pkg.INFO_PREPASS) == 3
    for lo in range(0, nb, per):
        if run == "digest":
            ptr, st, d = q.pop_digest()
            digs.append(d)
        else:
            ptr, st = q.pop()
        iqs.append(synth.device_read(ptr, (per, nsamp, 2)))
        sts.append(st)
    q.close()
    if run == "digest":
        dig = np.concatenate(digs)
    return np.concatenate(iqs), np.concatenate(sts), got, dig


def check(pkg, synth, oracle, case, run):
    name = "%s %s" % (case, run)
    ch, nsamp, want_iq, want_st, hz = wanted(pkg, oracle, case)
    rc, plan = pkg.plan(ch[:BPS], DELT, nsamp, flags=pkg.CHAIN_CARRIER)
    assert rc == 0 and plan["st_log2"] == 1 and plan["nstates"] == ((nsamp + TILE - 1) // TILE + 1) // 2, plan   # a granule table
    iq, st, got, dig = render(pkg, synth, ch, nsamp, run)
    print("%s: exact runs %d, itable_512 %d, dwrd_oob %d, tiles %d" % ((name,) + got))
    bad = np.nonzero((iq != want_iq).any(axis=(1, 2)))[0]
    assert bad.size == 0, (name, "blocks whose IQ differs", bad.tolist(), "first sample", int(np.nonzero((iq[bad[0]] != want_iq[bad[0]]).any(axis=1))[0][0]))
    assert tp.same_states(st, want_st, ch) == [], name
    if dig is not None:
        assert (dig == pkg.block_digest_host(want_iq)).all(), name
    assert (got[1], got[2]) == (int(hz["itable_512"]), int(hz["dwrd_oob"])), (name, got, hz)
    if run != "per-sample":
        assert got[3] == ch.shape[0] * ((nsamp + TILE - 1) // TILE), (name, got)
    assert got[:3] == tuple(PARENT[name]), (name, got, PARENT[name])


@pytest.fixture()
def fresh(pkg, synth):
    for opt in (pkg.OPT_SEED_WHERE, pkg.OPT_SYNTH_KERNEL, pkg.OPT_CHAIN_WHERE):
        synth.set_option(opt, 0)
    yield synth
    for opt in (pkg.OPT_SEED_WHERE, pkg.OPT_SYNTH_KERNEL, pkg.OPT_CHAIN_WHERE):
        synth.set_option(opt, 0)


def test_the_edges_are_where_they_were_put(pkg, oracle):
    """the oracle's end states say so: a channel with an edge ends the block under the other bit than it began it (one edge per
    block: 3 to 5 of a bit's 20 periods), one without under the same; and the blocks are 3 to 5 code periods long"""
    for case in ("edges-75000", "edges-125000"):
        ch, nsamp, _, st, _ = wanted(pkg, oracle, case)
        assert 3 <= nsamp // 25000 <= 5
        first = np.array([[1 if (int(ch["dwrd"][b, i, ch["iword"][b, i]]) >> (29 - int(ch["ibit"][b, i]))) & 1 else -1 for i in range(NCH)]
                          for b in range(ch.shape[0])])
        has_edge = np.array([E is not None for E in edges_of(nsamp)])
        assert (st["dataBit"][:, has_edge] == -first[:, has_edge]).all(), case
        assert (st["dataBit"][:, ~has_edge] == first[:, ~has_edge]).all(), case


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("case", list(CASES))
def test_against_the_oracle(pkg, fresh, oracle, case, run):
    check(pkg, fresh, oracle, case, run)
