"""The cache policy of the model kernels' IQ stores (gpsbb_events.hip.h iq_store: non-temporal or plain, GPSBB_IQ_NT) changes no
byte.  Whole tiles go out as four 1 KB stores per wavefront, a block's last, partial tile and every tile of a block that does not
start on 16 bytes go out sample by sample from the registers: both forms, k_synth_ev, its digest variant and k_synth_pd, through
batch.run and through a device-only ring, against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA")
RAGGED = 2 * 1024 + 16 + 3  # two whole tiles and 19 samples; 8268 bytes, so blocks 1 and 2 start 12 and 8 bytes past a 16-byte boundary
BPS = 3


def same_states(got, want):
    return all(got[f].tobytes() == want[f].tobytes() for f in FIELDS)


@pytest.fixture(scope="module")
def cases(pkg, oracle):
    """(descriptors of two pushes of three blocks, delt, nsamp, the oracle's chained IQ and end states), computed once"""
    out = {}
    for name, nch, fs, nsamp in (("ragged", 16, 25e6, RAGGED), ("whole", 16, 25e6, 4096), ("pd", 12, 2.6e6, 3000)):
        ch = pkg.synth_descriptors(2 * BPS, nch=nch, seed=0x1E + nsamp)
        iq, st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
        iq.setflags(write=False)
        st.setflags(write=False)
        out[name] = (ch, 1 / fs, nsamp, iq, st)
    return out


def variants_of(pkg, name):
    return (pkg.VARIANT_PD_WIDE, pkg.VARIANT_PD_NARROW) if name == "pd" else (pkg.VARIANT_EV,)


@pytest.mark.parametrize("name", ["ragged", "whole", "pd"])
def test_a_batch_is_the_oracles_bytes(pkg, synth, cases, name):
    ch, delt, nsamp, want_iq, want_st = cases[name]
    for opt in (pkg.OPT_SEED_WHERE, pkg.OPT_SYNTH_KERNEL, pkg.OPT_CHAIN_WHERE):
        synth.set_option(opt, 0)
    tiles0 = synth.info(pkg.INFO_TILES_RENDERED)
    b = synth.batch(ch[:BPS], delt, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    assert synth.info(pkg.INFO_LAST_KERNEL) == 2 and synth.info(pkg.INFO_LAST_VARIANT) in variants_of(pkg, name)
    assert synth.info(pkg.INFO_TILES_RENDERED) - tiles0 == BPS * ((nsamp + 1023) // 1024)
    assert (iq == want_iq[:BPS]).all()
    assert same_states(st, want_st[:BPS])


@pytest.mark.parametrize("name", ["ragged", "whole", "pd"])
def test_a_device_only_ring_is_the_oracles_bytes(pkg, synth, cases, name):
    """the first push plain, the second with GPSBB_PUSH_DIGEST: the digest variant's sums, taken from the registers, are those of
    the bytes its stores left in the slot"""
    ch, delt, nsamp, want_iq, want_st = cases[name]
    for opt in (pkg.OPT_SEED_WHERE, pkg.OPT_SYNTH_KERNEL, pkg.OPT_CHAIN_WHERE):
        synth.set_option(opt, 0)
    tiles0 = synth.info(pkg.INFO_TILES_RENDERED)
    ring = synth.stream(ch.shape[1], delt, nsamp, BPS, depth=2, flags=pkg.CHAIN_CARRIER | pkg.STREAM_DEVICE_ONLY)
    ring.push(ch[:BPS])
    ring.push(ch[BPS:], digest=True)
    assert synth.info(pkg.INFO_LAST_KERNEL) == 2 and synth.info(pkg.INFO_LAST_VARIANT) in variants_of(pkg, name)
    p0, st0 = ring.pop()
    iq0 = synth.device_read(p0, (BPS, nsamp, 2))
    p1, st1, dig = ring.pop_digest()
    iq1 = synth.device_read(p1, (BPS, nsamp, 2))
    of_slot = synth.device_digest(p1, BPS, nsamp)
    ring.close()
    assert synth.info(pkg.INFO_TILES_RENDERED) - tiles0 == 2 * BPS * ((nsamp + 1023) // 1024)
    assert (iq0 == want_iq[:BPS]).all() and (iq1 == want_iq[BPS:]).all()
    assert same_states(st0, want_st[:BPS]) and same_states(st1, want_st[BPS:])
    assert (dig == of_slot).all(), (dig, of_slot)
    assert (dig == pkg.block_digest_host(want_iq[BPS:])).all()
