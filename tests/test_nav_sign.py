"""The data bits of a granule table (ev_nav_in_sign, pluto-gps-sim_amd/csrc/gpsbb_events.hip.h), on the host: a table with one
exact state per 2^g tiles, g >= 1, has no tile_nav words — the sign of a code state says that the data bit in force at the
granule's first sample is -1, readers take the magnitude, and the bit after a roll-over inside entry e is the sign of entry e + 1
or, behind the row's last entry, the dataBit of the block's end state.  The rule as the library compiles it (gpsbb_test_nav_sign)
against a numpy restatement; and the plan's sizes, which the encoding must leave alone."""
import numpy as np
import pytest

SIGN = np.uint64(1) << np.uint64(63)
LARGEST = np.nextafter(np.float64(1023.0), np.float64(0.0))   # the largest code state there is


def states():
    rng = np.random.default_rng(0x4E56)
    x = np.concatenate([[0.0, LARGEST, np.nextafter(np.float64(0.0), np.float64(1.0)), 1.0, 512.0, 1022.0],
                        rng.uniform(0.0, 1023.0, 500), rng.uniform(0.0, 1.0, 50) * 2.0 ** rng.integers(-60, 0, 50)]).astype(np.float64)
    assert (x >= 0.0).all() and (x < 1023.0).all()
    return x


@pytest.mark.parametrize("g", [1, 2])
def test_the_bit_travels_in_the_sign(pkg, g):
    """magnitude and bit come back from what the table holds, for either bit; the 52-bit state is untouched, 0.0 becomes -0.0"""
    for x in states():
        bits = np.float64(x).view(np.uint64)
        for minus in (0, 1):
            stored, mag, bit, _, _, in_sign = pkg.nav_sign(x, minus, g)
            want = bits | SIGN if minus else bits                      # the numpy restatement: copysign
            assert in_sign
            assert stored == int(want) == int(np.copysign(x, -1.0 if minus else 1.0).view(np.uint64)), (x, minus)
            assert mag == int(bits) == int(np.abs(np.uint64(stored).view(np.float64)).view(np.uint64)), (x, minus)
            assert bit == minus == int(np.signbit(np.uint64(stored).view(np.float64))), (x, minus)
    stored, mag, bit, _, _, _ = pkg.nav_sign(0.0, 1, g)
    assert stored == int(SIGN) and np.uint64(stored).view(np.float64) == 0.0 and mag == 0 and bit == 1   # -0.0


def test_a_table_with_a_state_per_tile_keeps_plain_states(pkg):
    """g = 0 (every kernel but the breakpoint kernel behind the lap-parallel pre-pass): states as they are, the bits in tile_nav"""
    for x in states()[:40]:
        for minus in (0, 1):
            stored, mag, bit, _, _, in_sign = pkg.nav_sign(x, minus, 0)
            assert not in_sign and stored == mag == int(np.float64(x).view(np.uint64)) and bit == 0


@pytest.mark.parametrize("used", [1, 2, 37, 49, 611, 1221])
def test_where_the_next_bit_lies(pkg, used):
    """entry e + 1 of the row for every entry but the last one used, the block's end state behind that one"""
    for e in sorted({0, 1, used // 2, used - 2, used - 1} & set(range(used))):
        _, _, _, from_end, entry, _ = pkg.nav_sign(1.0, 0, 1, e, used)
        assert from_end == (e == used - 1), (e, used)
        assert entry == (-1 if e == used - 1 else e + 1), (e, used)


def test_the_plan_keeps_its_sizes(pkg):
    """nstates is ceil(ntiles / 2^st_log2) as before — no pad entry — and ntiles where st_log2 == 0"""
    ch = pkg.synth_descriptors(3, nch=16, seed=0x4E57)
    want = {}
    for nsamp in (1024, 2048, 2049, 75000, 100352, 125000):
        want[(25e6, nsamp, 0, 0)] = 1                       # k_synth_ev behind the lap-parallel pre-pass: one state per 2 tiles
        want[(25e6, nsamp, 1, 0)] = 0                       # ... behind the row walks: one per tile
        want[(25e6, nsamp, 0, pkg.FIXED_CARRIER)] = 0       # k_synth_ev_fixed
    want[(2.6e6, 300000, 0, 0)] = 0                         # k_synth_pd
    for (fs, nsamp, seed_where, flags), st_log2 in want.items():
        d = ch.copy()
        if flags & pkg.FIXED_CARRIER:
            d["carr_phase"] = 0.0
        rc, v = pkg.plan(d, 1.0 / fs, nsamp, flags=flags, seed_where=seed_where)
        assert rc == 0, (fs, nsamp, seed_where, flags, rc)
        assert v["st_log2"] == st_log2, (fs, nsamp, seed_where, flags, v["st_log2"])
        assert v["ntiles"] == (nsamp + 1023) // 1024
        assert v["nstates"] == (v["ntiles"] + (1 << st_log2) - 1) >> st_log2, (fs, nsamp, seed_where, flags, v)
        if st_log2 == 0:
            assert v["nstates"] == v["ntiles"]
