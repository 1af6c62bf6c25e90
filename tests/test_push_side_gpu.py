"""The side a ring's push chains its carrier on (tests/test_push_side.py holds plan_push_side to the same table without a GPU),
as the ring itself shows it: two pushes through a ring of depth 2 per row, after each what the handle reports of its last
launch — GPSBB_INFO_CHAIN_ON_DEVICE, and GPSBB_INFO_PREPASS (3 the lap-parallel pre-pass, 1 the row walks, 2 host threads) —
and every pop's IQ and end states against the oracle's render of the four to ten blocks as one chain.

  not chained, or the accumulator's chain     0, and whatever pre-pass the plan picks
  the device side, by the laps                1 and 3
  the device side, by the row walks           1 and 1
  the host side                               0, and 2 where the push is small enough to be seeded there too

Public API only: the table was validated on the commit before plan_push_side existed, where this file passes unchanged."""
import numpy as np
import pytest

import batch_plan_cases as bpc

pytestmark = pytest.mark.gpu

CHAIN, FIXED = bpc.CHAIN, bpc.FIXED
FIELDS = ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA")
SMALL, SMALL_1M, ODD_2M6 = (25e6, 4096), (1e6, 4096), (2.6e6, 4097)
# name: (blocks per push, nch), (sample rate, samples per block), flags, options, (chain on device, pre-pass)
ROWS = {
    "plain-small": ((2, 4), SMALL, 0, {}, (0, 3)),
    "fixed-chain-small": ((2, 4), SMALL, FIXED | CHAIN, {}, (0, 3)),
    "small-by-laps": ((2, 4), SMALL, CHAIN, {}, (1, 3)),
    "small-per-sample": ((2, 4), SMALL, CHAIN, dict(OPT_SYNTH_KERNEL=1), (0, 2)),
    "small-cw2": ((2, 4), SMALL, CHAIN, dict(OPT_CHAIN_WHERE=2), (0, 2)),
    "small-1M": ((2, 4), SMALL_1M, CHAIN, {}, (0, 2)),  # the model kernels decline 1 MS/s
    "64-per-sample": ((4, 16), ODD_2M6, CHAIN, dict(OPT_SYNTH_KERNEL=1), (0, 2)),
    "80-per-sample": ((5, 16), ODD_2M6, CHAIN, dict(OPT_SYNTH_KERNEL=1), (1, 1)),
    "80-row-walks": ((5, 16), ODD_2M6, CHAIN, dict(OPT_SEED_WHERE=1), (1, 1)),
    "80-chain-on-host": ((5, 16), ODD_2M6, CHAIN, dict(OPT_CHAIN_WHERE=1), (0, 3)),  # the host chains, the laps seed
}


@pytest.mark.parametrize("name", list(ROWS))
def test_ring_reports_the_side_and_renders_the_oracle_chain(pkg, synth, oracle, name):
    (bps, nch), (fs, nsamp), flags, opts, want_info = ROWS[name]
    ch = bpc.descriptors(np.random.default_rng(bpc.SEED), pkg, 2 * bps, nch, bool(flags & FIXED))
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=bool(flags & CHAIN), fixed=bool(flags & FIXED))
    try:
        for o, v in opts.items():
            synth.set_option(getattr(pkg, o), v)
        ring = synth.stream(nch, 1 / fs, nsamp, bps, depth=2, flags=flags)
        for k in range(2):
            ring.push(ch[k * bps:(k + 1) * bps])
            assert (synth.info(pkg.INFO_CHAIN_ON_DEVICE), synth.info(pkg.INFO_PREPASS)) == want_info, "push %d" % k
        for k in range(2):
            iq, st = ring.pop()
            lo, hi = k * bps, (k + 1) * bps
            active = ch["prn"][lo:hi] > 0
            for f in FIELDS:
                assert st[f][active].tobytes() == want_st[f][lo:hi][active].tobytes(), "push %d: %s" % (k, f)
            assert (iq == want_iq[lo:hi]).all(), "push %d: IQ" % k
        ring.close()
    finally:
        for o in opts:
            synth.set_option(getattr(pkg, o), 0)
