"""Parity of the HIP path (through the C ABI) with the CPU oracle and the committed golden vectors of the
real reference.  Everything here is bit-exact: int16 IQ, end-of-block doubles compared by their bytes."""
import hashlib
import os
import sys

import numpy as np
import pytest

import oracle_binding as ob
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def assert_state_equal(got, want, active):
    for f in ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA"):
        g, w = got[f][active], want[f][active]
        assert g.tobytes() == w.tobytes(), f


ONCE = "default"   # the mode in which the tests that run once run: no option set at all, what a host that sets none gets


@pytest.fixture(autouse=True, params=["default", "k_seed+auto", "host+auto", "k_seed+per-sample", "host+per-sample",
                                      "k_seed+auto+seqfix", "k_seed+per-sample+seqfix", "k_seed+auto+passA", "laps+auto"])
def seed_mode(pkg, synth, request):
    """Every test below runs nine ways: first with NO option set ("default": the library's own choices — the lap-parallel
    pre-pass wherever it is eligible, the model kernels wherever they are; the full-size and full-length runs, which run once,
    run in this mode), then with the choices forced.  The exact NCO pre-pass of a run is computed on the device — by the row walks of
    rounds 1-4 (k_seed / k_walk + the chain kernels: "k_seed") or lap-parallel (gpsbb_laps.hip.h, round 5: "laps"; what the
    library picks by itself for anything but a handful of blocks) — or,
    for small batches, by host threads running the same code (by default the batch size decides); the
    synthesis kernel is chosen automatically (the model-based kernels k_synth_ev / k_synth_ev_dense wherever they are
    eligible: sample rates above ~2 MS/s) or forced to the per-sample kernel k_synth; and the last step of the
    device-side carrier chain takes the blocks in parallel (k_chain_fix_par, the default) or in order (k_chain_fix); and
    the start phases its one walk (pass B) begins from come from the host's drift model (the default) or from a first
    walk (pass A + k_chain_prefix)."""
    if request.param != "default":
        where, kernel = request.param.split("+")[:2]
        synth.set_option(pkg.OPT_SEED_WHERE, {"k_seed": 1, "host": 2, "laps": 3}[where])
        synth.set_option(pkg.OPT_SYNTH_KERNEL, 1 if kernel == "per-sample" else 0)
        synth.set_option(pkg.OPT_CHAIN_WHERE, 2 if request.param.endswith("seqfix") else (3 if request.param.endswith("passA") else 0))
    yield
    synth.set_option(pkg.OPT_SEED_WHERE, 0)
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 0)
    synth.set_option(pkg.OPT_CHAIN_WHERE, 0)


def mode_of(request):
    """(where, kernel) of the running mode; "default" reads as the library's own choices"""
    m = request.node.callspec.params["seed_mode"]
    return ("auto", "auto") if m == "default" else tuple(m.split("+")[:2])


def test_native_library_is_what_runs(pkg, synth):
    """The loaded shared object is the in-tree HIP build and it owns a device handle."""
    maps = open("/proc/self/maps").read()
    assert os.path.join("pluto-gps-sim_amd", "libgpsbb.so") in maps
    assert synth._h


@pytest.mark.parametrize("name", ["static_F", "motion_F", "dense_S", "loop_M2"])
def test_golden_vectors_of_the_real_reference(pkg, synth, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    fs, nsamp = float(z["fs"]), int(z["nsamp"])
    desc = z["desc"].view(pkg.CHAN_DTYPE).reshape(z["desc"].shape[0], -1)
    want_st = z["end_state"].view(pkg.STATE_DTYPE).reshape(desc.shape)
    for k in range(desc.shape[0]):
        iq, st = synth.fill_block(desc[k], 1.0 / fs, nsamp)
        assert (iq[:z["iq_prefix"].shape[1]] == z["iq_prefix"][k]).all(), (name, k)
        assert sha(iq) == str(z["iq_sha256"][k]), (name, k)
        assert_state_equal(st, want_st[k], desc["prn"][k] > 0)
    assert synth.hazards(reset=True) == {"itable_512": 0, "dwrd_oob": 0}


@pytest.mark.parametrize("fs,nsamp,nch,seed", [
    (25e6, 1, 16, 11), (25e6, 15, 16, 12), (25e6, 16, 16, 13), (25e6, 17, 3, 14), (2.6e6, 4095, 12, 15),
    (2.6e6, 4096, 12, 16), (2.6e6, 4097, 12, 17), (1e6, 100003, 16, 18), (3e6, 300000, 12, 19),
    (4.092e6, 65537, 1, 20), (25e6, 262146, 16, 21)])
def test_single_block_vs_oracle(pkg, synth, oracle, fs, nsamp, nch, seed):
    ch = pkg.synth_descriptors(1, nch=nch, seed=seed)[0]
    want_iq, want_st, hz = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
    iq, st = synth.fill_block(ch, 1.0 / fs, nsamp)
    assert (iq == want_iq[0]).all()
    assert_state_equal(st, want_st[0], ch["prn"] > 0)


def test_high_doppler_and_slow_channels(pkg, synth, oracle):
    """Row-table stress: the largest carrier steps of the contract, tiny ones, zero, both signs, and a step
    whose mantissa is a single bit (every addition is a rounding tie)."""
    fs, nsamp = 1e6, 50000
    ch = pkg.synth_descriptors(1, nch=10, seed=31)[0]
    ch["f_carr"] = [124999.0, -124999.0, 0.0, 1e-7, -1e-7, fs * 2.0 ** -10, -fs * 2.0 ** -10, 5000.0, -5000.0, 0.3]
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
    iq, st = synth.fill_block(ch, 1.0 / fs, nsamp)
    assert (iq == want_iq[0]).all()
    assert_state_equal(st, want_st[0], ch["prn"] > 0)


def test_carrier_steps_the_breakpoint_kernel_always_recomputes(pkg, synth, oracle, request):
    """At 25 MS/s the breakpoint kernel takes the block.  A carrier whose step per sample is below eight times the in-tile
    model's error has no usable model (EvConst::kc = -1): its threshold is one no low word is above (danger_le = 0xffffffff)
    and every lane-run goes through the exact path; a carrier that does not move at all has no index change to place.  Beside
    ordinary channels of both signs, in one batch."""
    fs, nsamp = 25e6, 120000
    ch = pkg.synth_descriptors(2, nch=12, seed=77)
    for b in range(2):
        ch[b]["f_carr"] = [0.0, 1e-5, -1e-5, 3e-4, -3e-4, 2e-3, -2e-3, 4999.0, -4999.0, 1200.0, -0.0, 5e-324]
        ch[b]["f_code"] = 1.023e6 + ch[b]["f_carr"] / 1540.0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
    b = synth.batch(ch, 1.0 / fs, nsamp)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    assert (iq == want_iq).all()
    for k in range(2):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    if "per-sample" not in request.node.callspec.params["seed_mode"]:
        assert synth.info(pkg.INFO_LAST_KERNEL) == 2  # the breakpoint kernel
        assert synth.info(pkg.INFO_EXACT_RUNS) >= 2 * 4 * (nsamp // 16)  # four always-exact channels per block at least


def test_steps_that_hit_chip_and_table_boundaries_exactly(pkg, synth, oracle):
    """Sample rates at which a run of 16 samples holds at most one chip boundary take the path that locates
    the boundary instead of stepping the code NCO.  With f_code*delt and f_carr*delt binary fractions the
    phases land exactly on integers / table-index boundaries, the case the locating division must settle
    with its exact check; start phases on and next to boundaries, both Doppler signs, two block lengths."""
    fs = 2.0 ** 25
    for nsamp, seed in ((70001, 41), (1 << 17, 42)):
        ch = pkg.synth_descriptors(1, nch=16, seed=seed)[0]
        ch["f_code"] = [2.0 ** 20, 2.0 ** 20, 2.0 ** 20, 2.0 ** 20 + 2.0 ** 10, 2.0 ** 20 - 2.0 ** 9, 2.0 ** 19,
                        2.0 ** 20, 1.023e6, 2.0 ** 20, 2.0 ** 20, 3.0 * 2.0 ** 18, 2.0 ** 20, 2.0 ** 20, 2.0 ** 20,
                        2.0 ** 20 + 1.0, 2.0 ** 21 - 2.0 ** 12]
        ch["code_phase"] = [0.0, 5.0, 1022.96875, 7.5, 100.0, 1022.5, 2.0 ** -5, 511.0, 1.0 - 2.0 ** -5, 512.0,
                            3.0, 1022.0, 0.5, 64.0, 255.0, 1000.0]
        ch["f_carr"] = [2.0 ** 12, -2.0 ** 12, 2.0 ** 11, -2.0 ** 11, 2.0 ** 14, -2.0 ** 14, 3.0 * 2.0 ** 10, 0.0,
                        2.0 ** 16, -2.0 ** 16, 2.0 ** 12, 2.0 ** 12, -2.0 ** 12, 2.0 ** 8, -2.0 ** 8, 2.0 ** 12 + 1.0]
        ch["carr_phase"] = [0.0, 0.0, 0.5, 1.0 / 512, 1.0 - 1.0 / 512, 2.0 ** -13, 0.25, 0.75, 0.0, 0.5,
                            1.0 - 2.0 ** -13, 2.0 ** -9, 511.0 / 512, 0.125, 0.375, 0.0]
        want_iq, want_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
        iq, st = synth.fill_block(ch, 1.0 / fs, nsamp)
        assert (iq == want_iq[0]).all(), nsamp
        assert_state_equal(st, want_st[0], ch["prn"] > 0)


def test_inactive_and_empty_channels(pkg, synth, oracle):
    ch = pkg.synth_descriptors(1, nch=8, seed=41)[0]
    ch["prn"][[1, 4, 7]] = 0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / 2.6e6, 20000)
    iq, st = synth.fill_block(ch, 1 / 2.6e6, 20000)
    assert (iq == want_iq[0]).all()
    assert_state_equal(st, want_st[0], ch["prn"] > 0)
    ch["prn"][:] = 0                      # nothing allocated: the reference writes zeros (c:2691-2692, 2754)
    iq, _ = synth.fill_block(ch, 1 / 2.6e6, 5000)
    assert not iq.any()


def test_large_gain_wraps_like_the_short_cast(pkg, synth, oracle):
    """(short)i_acc truncates modulo 2^16 (plutogpssim.c:2754-2755); gains far above the physical range
    make the accumulators overflow int16 and must still match."""
    ch = pkg.synth_descriptors(1, nch=16, seed=51)[0]
    ch["gain"] = np.linspace(20.0, 900.0, 16)
    ch["gain"][3] = -77.5
    want_iq, _, _ = oracle.fill_blocks(ch, 1 / 25e6, 30000)
    iq, _ = synth.fill_block(ch, 1 / 25e6, 30000)
    assert (iq == want_iq[0]).all()


def test_hazards_are_defined_and_counted_like_the_oracle(pkg, synth, oracle):
    synth.hazards(reset=True)
    ch = pkg.synth_descriptors(1, nch=2, seed=61)[0]
    ch["carr_phase"][0] = 1.0
    ch["f_carr"][0] = -100.0
    ch["iword"][1], ch["ibit"][1], ch["icode"][1] = 59, 29, 19
    want_iq, want_st, hz = oracle.fill_blocks(ch, 1 / 1e6, 100000)
    iq, st = synth.fill_block(ch, 1 / 1e6, 100000)
    assert (iq == want_iq[0]).all()
    assert_state_equal(st, want_st[0], ch["prn"] > 0)
    got = synth.hazards(reset=True)
    assert got == {"itable_512": int(hz["itable_512"]), "dwrd_oob": int(hz["dwrd_oob"])}
    assert got["itable_512"] == 1 and got["dwrd_oob"] == 5


def test_contract_violations_return_badchan(pkg, synth):
    ch = pkg.synth_descriptors(1, nch=2, seed=71)[0]
    for field, val in [("code_phase", 1023.0), ("carr_phase", -0.1), ("carr_phase", 1.5), ("prn", 40),
                       ("gain", float("inf")), ("iword", 60), ("f_code", 0.0), ("f_carr", 2e6)]:
        bad = ch.copy()
        bad[field][0] = val
        with pytest.raises(pkg.GpsbbError) as e:
            synth.fill_block(bad, 1 / 2.6e6, 100)
        assert e.value.rc == -2, field


def test_batch_independent_blocks(pkg, synth, oracle):
    ch = pkg.synth_descriptors(5, nch=16, seed=81)
    ch["prn"][2, 5] = 0
    delt, nsamp = 1 / 25e6, 70001
    want_iq, want_st, _ = oracle.fill_blocks(ch, delt, nsamp, chain=False)
    b = synth.batch(ch, delt, nsamp)
    assert b.iq_bytes == 5 * nsamp * 4
    b.run()
    synth.sync()
    iq, st = b.read()
    assert (iq == want_iq).all()
    for k in range(5):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    t = b.timing()
    assert t["ms_synth"] > 0 and t["ms_total"] >= t["ms_synth"]
    b.run()                                 # a batch can be re-run
    synth.sync()
    assert (b.read()[0] == want_iq).all()
    b.close()


def test_batch_chained_carrier(pkg, synth, oracle):
    """GPSBB_CHAIN_CARRIER: block b continues block b-1's carrier phase on the device, like iterating
    plutogpssim.c:2655; a re-allocated channel restarts from its own descriptor."""
    ch = pkg.synth_descriptors(6, nch=12, seed=91)
    ch["prn"][3:, 4] = 30
    ch["prn"][2, 7] = 0
    delt, nsamp = 1 / 2.6e6, 300000
    want_iq, want_st, _ = oracle.fill_blocks(ch, delt, nsamp, chain=True)
    b = synth.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    assert (iq == want_iq).all()
    for k in range(6):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    # the host chaining helper gives the same seeds, so time shards can start anywhere
    seeds = pkg.chain_carrier_host(ch, delt, nsamp)
    ch2 = ch.copy()
    ch2["carr_phase"] = seeds
    b2 = synth.batch(ch2[3:], delt, nsamp)  # "GPU 1" gets blocks 3..5 only
    b2.run()
    synth.sync()
    assert (b2.read()[0] == want_iq[3:]).all()
    b.close()
    b2.close()



def test_carrier_chained_on_the_device(pkg, synth, oracle, request):
    """GPSBB_CHAIN_CARRIER at a sample rate the breakpoint kernel takes: the exact carrier chain runs on the
    device, in parallel over the blocks (pass A, prefix, pass B, k_chain_fix: every block is walked from a
    start phase a few units in the last place off and shifted onto the true trajectory after its first wrap).
    Bit-exact against the oracle walking the blocks in order, for every kind of block the fix-up knows:
    translated ones, channels too slow to wrap within a block (walked sequentially), a step that can tie,
    a channel that does not move, channels that come and go."""
    nb, nch = 24, 16
    fs, nsamp = 25e6, 120000
    ch = pkg.synth_descriptors(nb, nch=nch, seed=4242)
    rng = np.random.default_rng(5)
    # one Doppler per channel, drifting a little from block to block like a real pass
    f0 = rng.uniform(-5000, 5000, nch)
    f0[0], f0[1], f0[2], f0[3] = 3.0, -40.0, 0.0, fs * 2.0 ** -14       # no wrap in a block / none ever / tie-prone step
    ch["f_carr"] = f0[None, :] + rng.uniform(-0.5, 0.5, (nb, nch)) * (np.abs(f0[None, :]) > 100)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    ch["prn"] = np.arange(1, nch + 1)[None, :]
    ch["prn"][7:, 5] = 31        # channel 5 re-allocated at block 7: restarts from its descriptor
    ch["prn"][10:13, 9] = 0      # channel 9 off for three blocks
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    fb0 = synth.info(pkg.INFO_CHAIN_FALLBACKS)
    b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    for _ in range(2):           # two runs: the table sets alternate
        b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    where, kernel = mode_of(request)
    if where == "k_seed" and kernel == "auto":
        assert synth.info(pkg.INFO_LAST_KERNEL) == 2 and synth.info(pkg.INFO_CHAIN_ON_DEVICE) == 1
        # blocks the fix-up had to walk sequentially: at most those of the four special channels (often fewer:
        # where pass A's prediction of a start phase is exact to the bit there is nothing to fix) plus a few
        fb = synth.info(pkg.INFO_CHAIN_FALLBACKS) - fb0
        assert fb <= 2 * (4 * (nb - 1) + 12), fb
    assert (iq == want_iq).all()
    for k in range(nb):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    # ... and forced onto host threads it is the same bytes
    synth.set_option(pkg.OPT_CHAIN_WHERE, 1)
    try:
        b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
        b.run()
        synth.sync()
        assert synth.info(pkg.INFO_CHAIN_ON_DEVICE) == 0
        assert (b.read()[0] == want_iq).all()
        b.close()
    finally:
        synth.set_option(pkg.OPT_CHAIN_WHERE, 0)


def test_stream_ring_with_pinned_gather(pkg, synth, oracle):
    nch, delt, nsamp, bps = 8, 1 / 4.092e6, 50000, 2
    ch = pkg.synth_descriptors(10, nch=nch, seed=101)
    want_iq, want_st, _ = oracle.fill_blocks(ch, delt, nsamp, chain=True)
    s = synth.stream(nch, delt, nsamp, bps, depth=3, flags=pkg.CHAIN_CARRIER)
    got = []
    for k in range(5):
        if s.pending == 3:
            got.append(s.pop())
        s.push(ch[2 * k:2 * k + 2])
    with pytest.raises(pkg.GpsbbError):
        while True:
            s.push(ch[0:2])                 # ring full -> GPSBB_E_STATE
    while s.pending:
        got.append(s.pop())
    got = got[:5]
    iq = np.concatenate([g[0] for g in got])
    st = np.concatenate([g[1] for g in got])
    assert (iq == want_iq).all()
    for k in range(10):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    s.close()




def test_device_chain_through_wraps_that_tie(pkg, synth, oracle, request):
    """Falling carriers at high Doppler over full-size blocks: ~750 wraps per block and channel, and about one in
    8000 of them adds 1.0 to a phase whose low bits put the sum exactly half-way between two doubles.  Such a tie
    goes to the even neighbour — a different one for the true trajectory than for pass B's when they are an odd
    number of grid steps apart — so pass B has to find and record them and k_chain_fix has to step through them.
    Bit-exact end states and IQ against the oracle walking the blocks in order."""
    nb, nch = 8, 16
    fs, nsamp = 25e6, 2500000
    ch = pkg.synth_descriptors(nb, nch=nch, seed=2718)
    rng = np.random.default_rng(11)
    ch["f_carr"] = -rng.uniform(3000.0, 12000.0, nch)[None, :] + rng.uniform(-0.5, 0.5, (nb, nch))
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    ties0 = synth.info(pkg.INFO_CHAIN_TIES)
    b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    where, kernel = mode_of(request)
    if where == "k_seed" and kernel == "auto":
        assert synth.info(pkg.INFO_CHAIN_ON_DEVICE) == 1
        # the first tie after a block's first wrap is recorded (later ones cannot matter): the case is really exercised,
        # and the fix-up did not have to walk blocks on its own because of it
        assert synth.info(pkg.INFO_CHAIN_TIES) - ties0 >= 3
    for k in range(nb):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    assert sha(iq) == sha(want_iq)



def test_device_chain_with_steps_that_tie_on_the_coarsest_grid(pkg, synth, oracle, request):
    """Carrier steps built bit by bit (fs = 2^25, so f_carr*delt is exact): multiples of 2^-53 and of 2^-52 (a rising
    phase's wrap sums are then exact or exact ties), odd multiples of 2^-54 (a falling phase then ties at every step
    in the top binade), and their neighbours.  Chained over 12 blocks; bit-exact against the oracle."""
    fs, nsamp, nb, nch = 2.0 ** 25, 300000, 12, 16
    ch = pkg.synth_descriptors(nb, nch=nch, seed=99)
    k = np.array([1801439850948, 1801439850949, 3602879701896, 3602879701897, 901439850951, 1201439850950,
                  2201439850947, 1501439850952], dtype=np.float64)          # ~1e-4 .. 4e-4 cycles per sample
    s = np.concatenate([k[:4] * 2.0 ** -53, k[4:] * 2.0 ** -52, -(2 * k[:4] + 1) * 2.0 ** -54, -k[4:] * 2.0 ** -53])
    ch["f_carr"] = (s * fs)[None, :]
    assert ((ch["f_carr"][0] * (1.0 / fs)) == s).all()
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    for j in range(nb):
        assert_state_equal(st[j], want_st[j], ch["prn"][j] > 0)
    assert (iq == want_iq).all()


def test_device_chain_step_that_ties_one_binade_up(pkg, synth, oracle):
    """Found by the batch soak (tools/fuzz_parity.py --seed 401, case 138) once pass B's start phases came from the drift
    model: a rising carrier with a large step (0.063 cycles per sample) whose mantissa is odd starts a block ONE binade
    above the step — there every sum x + s is an exact tie, and a start phase an odd number of last places away from the
    true one rounds every one of them the other way.  The fix-up has to walk that first lap (it used to look for tie-prone
    binades from two above the step only).  Two chained blocks of nine channels at 3 MS/s, bit-exact."""
    ch = np.load(os.path.join(GOLDEN, "chain_model_big_step_desc.npy"))
    fs, nsamp = 3e6, 10240
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    for k in range(ch.shape[0]):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    assert (iq == want_iq).all()


@pytest.mark.parametrize("fixture,fs,nsamp,bps", [("chain_first_wrap_tie_desc.npy", 30e6, 24607, 33),
                                                  ("chain_prefix_then_tie_desc.npy", 50e6, 3507, 100)])
def test_device_chain_cases_found_by_the_stream_soak(pkg, synth, oracle, request, fixture, fs, nsamp, bps):
    """Two single-channel streams on which the device-side chain was once off by one grid step (tools/fuzz_parity.py
    --stream).  (1) A falling carrier whose pass B starts half a step of the coarsest grid below the true phase: at
    the block's first wrap pass B's "+ 1.0" is an exact tie while the true sum lands on a grid point, which leaves the
    two an ODD number of grid steps apart — so the tie at the block's second wrap still changes the offset and has to
    be recorded.  (2) A block whose first lap k_chain_fix walks on its own (a tie-prone binade on the way up) and
    that has a tie at a later wrap: the crossings pass B recorded after the first wrap count on that path too.
    Pushed through a ring as they failed; bit-exact end states and IQ."""
    ch = np.load(os.path.join(GOLDEN, fixture))
    nb = ch.shape[0]
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    for depth in (2, 4):
        st_ = synth.stream(1, 1 / fs, nsamp, bps, depth=depth, flags=pkg.CHAIN_CARRIER)
        got, gst = [], []
        for k in range(nb // bps):
            if st_.pending == depth:
                a, b = st_.pop()
                got.append(a), gst.append(b)
            st_.push(ch[k * bps:(k + 1) * bps])
        while st_.pending:
            a, b = st_.pop()
            got.append(a), gst.append(b)
        st_.close()
        gst = np.concatenate(gst)
        for k in range(nb):
            assert_state_equal(gst[k], want_st[k], ch["prn"][k] > 0)
        assert (np.concatenate(got) == want_iq).all()
    # and as one batch
    b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    for k in range(nb):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    assert (iq == want_iq).all()


def test_stream_carrier_carried_on_the_device(pkg, synth, oracle, request):
    """A chained stream at 25 MS/s: the exact carrier phase is carried from push to push in device memory (no host
    chain), channels come and go between pushes, and the bytes are those of the oracle walking all blocks in
    order.  Also with the ring rendering into HBM only (STREAM_DEVICE_ONLY)."""
    nch, fs, nsamp, bps, npush = 16, 25e6, 60000, 5, 6
    ch = pkg.synth_descriptors(bps * npush, nch=nch, seed=777)
    ch["prn"] = np.arange(1, nch + 1)[None, :]
    f0 = np.linspace(-4800, 4800, nch)
    f0[3], f0[8] = 2.0, 0.0
    ch["f_carr"] = f0[None, :]
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    ch["prn"][bps * 2:, 6] = 29            # re-allocated exactly at a push boundary
    ch["prn"][bps * 3 + 2:bps * 4 + 1, 11] = 0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    where, kernel = mode_of(request)
    for flags in (pkg.CHAIN_CARRIER, pkg.CHAIN_CARRIER | pkg.STREAM_DEVICE_ONLY):
        st_ = synth.stream(nch, 1 / fs, nsamp, bps, depth=3, flags=flags)
        got, gst = [], []
        for k in range(npush):
            if st_.pending == 3:
                a, b = st_.pop()
                got.append(a), gst.append(b)
            st_.push(ch[k * bps:(k + 1) * bps])
        while st_.pending:
            a, b = st_.pop()
            got.append(a), gst.append(b)
        if where == "k_seed" and kernel == "auto":
            assert synth.info(pkg.INFO_CHAIN_ON_DEVICE) == 1
        gst = np.concatenate(gst)
        for k in range(bps * npush):
            assert_state_equal(gst[k], want_st[k], ch["prn"][k] > 0)
        if not (flags & pkg.STREAM_DEVICE_ONLY):
            assert (np.concatenate(got) == want_iq).all()
        st_.close()


def test_external_device_buffer(pkg, synth, oracle):
    import torch
    ch = pkg.synth_descriptors(2, nch=16, seed=111)
    delt, nsamp = 1 / 25e6, 40000
    out = torch.zeros(2 * nsamp * 2, dtype=torch.int16, device="cuda:0")
    b = synth.batch(ch, delt, nsamp)
    b.run(out.data_ptr())
    synth.sync()
    want_iq, _, _ = oracle.fill_blocks(ch, delt, nsamp)
    assert (out.cpu().numpy().reshape(2, nsamp, 2) == want_iq).all()
    b.close()


def test_reference_struct_layout_entry_point(pkg, synth, oracle):
    """gpsbb_fill_block_ref: the caller keeps the reference's channel_t (plutogpssim.h:152-174); build that
    layout here (LP64: int prn; int ca[1023]; double f_carr, f_code, carr_phase, code_phase; gpstime_t g0;
    unsigned long sbf[5][10]; unsigned long dwrd[60]; int iword, ibit, icode, dataBit, codeCA; ...)."""
    import ctypes as C
    from conftest import REF_CHANNEL_DTYPE as chan_t   # checked against offsetof() on the real header: test_ref_layout.py
    d = pkg.synth_descriptors(1, nch=12, seed=121)[0]
    d["prn"][5] = 0
    chan = np.zeros(12, chan_t)
    for f in ("prn", "f_carr", "f_code", "carr_phase", "code_phase", "iword", "ibit", "icode"):
        chan[f] = d[f]
    chan["dwrd"] = d["dwrd"]
    gain = np.ascontiguousarray(d["gain"])

    class Layout(C.Structure):
        _fields_ = [(n, C.c_size_t) for n in ("stride", "off_prn", "off_f_carr", "off_f_code", "off_carr_phase",
                                              "off_code_phase", "off_dwrd", "sizeof_dwrd_elem", "off_iword",
                                              "off_ibit", "off_icode", "off_dataBit", "off_codeCA")]
    off = lambda n: chan_t.fields[n][1]
    lay = Layout(chan_t.itemsize, off("prn"), off("f_carr"), off("f_code"), off("carr_phase"), off("code_phase"),
                 off("dwrd"), 8, off("iword"), off("ibit"), off("icode"), off("dataBit"), off("codeCA"))
    nsamp, delt = 300000, 1 / 2.6e6
    iq = np.zeros((nsamp, 2), np.int16)
    rc = pkg.lib().gpsbb_fill_block_ref(synth._h, chan.ctypes.data, C.byref(lay), 12, gain.ctypes.data, delt,
                                        nsamp, iq.ctypes.data)
    assert rc == 0
    want_iq, want_st, _ = oracle.fill_blocks(d, delt, nsamp)
    assert (iq == want_iq[0]).all()
    act = d["prn"] > 0
    for f in ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA"):
        assert chan[f][act].tobytes() == want_st[f][0][act].astype(chan[f].dtype).tobytes(), f


def test_a_registered_iq_buff_is_rendered_into(pkg, synth, oracle):
    """gpsbb_host_register: the reference's iq_buff is one calloc for the life of the process (c:2604, freed c:2815); registered
    once, the fill calls render straight into it (the synthesis kernel's stores cross the bus; no copy ends the call).  The bytes
    are the oracle's whichever way they arrive: a block at the start of the registered range, one at an odd offset inside it, one
    that starts inside it and ends beyond (copied, like one that lies outside altogether), the reference geometry, the
    headline's, the per-sample kernel; nothing outside the block is touched; the state comes back as always.  Overlapping
    registrations and unknown pointers are refused, and an unregistered buffer is copied into again."""
    L = pkg.lib()
    buf = np.zeros((700001, 2), np.int16)                 # "iq_buff", of which the first 500 000 samples are registered
    nreg = 500000
    assert L.gpsbb_host_register(synth._h, buf.ctypes.data, nreg * 4) == 0
    lay = pkg.ref_layout()

    def check(nch, fs, nsamp, at, seed):
        d = pkg.synth_descriptors(1, nch=nch, seed=seed)
        chan, gain = pkg.ref_channels(d[0])
        want_iq, want_st, _ = oracle.fill_blocks(d, 1.0 / fs, nsamp)
        buf[:] = 0x5a5a
        iq = buf[at:at + nsamp]
        synth.fill_block_ref(chan, gain, 1.0 / fs, nsamp, iq, lay)
        assert (iq == want_iq[0]).all(), (nch, fs, nsamp, at)
        assert (buf[:at] == 0x5a5a).all() and (buf[at + nsamp:] == 0x5a5a).all()
        act = d["prn"][0] > 0
        for f in ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA"):
            assert chan[f][act].tobytes() == want_st[f][0][act].astype(chan[f].dtype).tobytes(), f

    try:
        assert L.gpsbb_host_register(synth._h, buf.ctypes.data + 4096, 8192) == -7      # GPSBB_E_STATE: overlaps
        assert L.gpsbb_host_register(synth._h, buf.ctypes.data - 64, 128) == -7
        assert L.gpsbb_host_unregister(synth._h, buf.ctypes.data + 4096) == -7          # not the start of a range
        for case in ((12, 2.6e6, 300000, 0, 5), (12, 2.6e6, 300000, 333, 6), (12, 2.6e6, nreg - 333, 333, 10), (16, 25e6, 400000, 1001, 7),
                     (12, 2.6e6, 300000, 400000, 8), (12, 2.6e6, 200000, nreg, 11), (3, 1.0e6, 50000, 17, 9)):
            check(*case)
    finally:
        assert L.gpsbb_host_unregister(synth._h, buf.ctypes.data) == 0
    assert L.gpsbb_host_unregister(synth._h, buf.ctypes.data) == -7                     # gone
    check(12, 2.6e6, 300000, 0, 5)                                                      # ... and copied into, as before


def test_reference_struct_layout_entry_point_without_float_carr_phase(pkg, synth, oracle):
    """gpsbb_fill_block_ref_fixed: the caller keeps the channel_t of a reference built without FLOAT_CARR_PHASE (h:12
    removed; h:160-161: `unsigned int carr_phase; int carr_phasestep;`).  Two consecutive blocks through the struct, the
    accumulator updated in place in between like the loop does (c:2748); a host whose carr_phasestep is not the step of
    c:2675 is refused."""
    import ctypes as C
    from conftest import REF_CHANNEL_FIXED_DTYPE as chan_t   # checked against offsetof() on the real header: test_ref_layout.py
    nsamp, delt = 300000, 1 / 2.6e6
    d = _fixed_desc(pkg, 2, 12, 122)
    d["prn"][:, 7] = 0
    d[1] = d[0]
    chan = np.zeros(12, chan_t)
    for f in ("prn", "f_carr", "f_code", "code_phase", "iword", "ibit", "icode"):
        chan[f] = d[f][0]
    chan["carr_phase"] = d["carr_phase"][0].astype(np.uint32)
    chan["carr_phasestep"] = np.round(512.0 * 65536.0 * d["f_carr"][0] * delt).astype(np.int32)
    chan["dwrd"] = d["dwrd"][0]
    gain = np.ascontiguousarray(d["gain"][0])

    class Layout(C.Structure):
        _fields_ = [(n, C.c_size_t) for n in ("stride", "off_prn", "off_f_carr", "off_f_code", "off_carr_phase",
                                              "off_code_phase", "off_dwrd", "sizeof_dwrd_elem", "off_iword",
                                              "off_ibit", "off_icode", "off_dataBit", "off_codeCA")]
    off = lambda n: chan_t.fields[n][1]
    lay = Layout(chan_t.itemsize, off("prn"), off("f_carr"), off("f_code"), off("carr_phase"), off("code_phase"),
                 off("dwrd"), 8, off("iword"), off("ibit"), off("icode"), off("dataBit"), off("codeCA"))
    want_iq, want_st, _ = oracle.fill_blocks(d, delt, nsamp, chain=True, fixed=True)
    act = d["prn"][0] > 0
    for blk in range(2):
        iq = np.zeros((nsamp, 2), np.int16)
        rc = pkg.lib().gpsbb_fill_block_ref_fixed(synth._h, chan.ctypes.data, C.byref(lay), off("carr_phasestep"), 12,
                                                  gain.ctypes.data, delt, nsamp, iq.ctypes.data)
        assert rc == 0
        assert (iq == want_iq[blk]).all(), blk
        assert (chan["carr_phase"][act] == want_st["carr_phase"][blk][act].astype(np.uint32)).all()
        for f in ("code_phase", "iword", "ibit", "icode", "dataBit", "codeCA"):
            assert chan[f][act].tobytes() == want_st[f][blk][act].astype(chan[f].dtype).tobytes(), f
        # the host's per-block update (computeCodePhase, c:2673) puts the descriptor's values back; the accumulator stays
        for f in ("code_phase", "iword", "ibit", "icode"):
            chan[f] = d[f][1]
    chan["carr_phasestep"][0] += 1
    iq = np.zeros((nsamp, 2), np.int16)
    assert pkg.lib().gpsbb_fill_block_ref_fixed(synth._h, chan.ctypes.data, C.byref(lay), off("carr_phasestep"), 12,
                                                gain.ctypes.data, delt, nsamp, iq.ctypes.data) == -2
    assert pkg.lib().gpsbb_fill_block_ref_fixed(synth._h, chan.ctypes.data, C.byref(lay), C.c_size_t(-1).value, 12,
                                                gain.ctypes.data, delt, nsamp, iq.ctypes.data) == 0


def test_full_size_blocks_and_linearity(pkg, synth, oracle):
    """BASELINE config 3 size (16 channels, 25 MS/s, 2.5 M samples per block): two blocks compared sample
    for sample with the oracle, plus the size-independent property that the sum over channels is linear
    modulo 2^16: all channels together == sum of each channel alone."""
    delt, nsamp = 1 / 25e6, 2500000
    ch = pkg.synth_descriptors(2, nch=16, seed=0x5EED)
    b = synth.batch(ch, delt, nsamp)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    want_iq, want_st, _ = oracle.fill_blocks(ch, delt, nsamp)
    assert (iq == want_iq).all()
    for k in range(2):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    total = np.zeros((nsamp, 2), np.int16)
    for i in range(16):
        one = ch[0].copy()
        one["prn"][np.arange(16) != i] = 0
        part, _ = synth.fill_block(one, delt, nsamp)
        total += part                        # int16 wrap-around addition
    assert (total == iq[0]).all()


@pytest.mark.parametrize("name,nav,motion,max_chan,kw", [
    ("static_F", "synth3540.14n", None, 12, {}),            # BASELINE configs 1/2
    ("motion_F", "synth3540.14n", "circle_motion.csv", 12, {}),   # config 4: 10 Hz user motion
    ("dense_S", "dense3540.14n", None, 16, {}),             # config 3 geometry through the front end
    ("rinex3_F", "synth3540_v3.rnx", None, 12, {"rinex3": True}),                  # readRinex3, c:1241-1610
    ("toverwrite_F", "synth3540.14n", None, 12, {"start": (2014, 12, 21, 10, 0, 0.0), "time_overwrite": True}),  # -T
    ("motion_ref_F", "synth3540.14n", "circle.csv", 12, {}),                       # config 4 on the reference's circle.csv
    ("swap_S", "dense3540.14n", None, 16, {"start": (2014, 12, 20, 1, 20, 0.0)})])  # a channel changes hands at block 1500
def test_end_to_end_from_rinex(pkg, synth, name, nav, motion, max_chan, kw):
    """RINEX file + position/motion -> from-scratch host front end -> device (carrier chained on the GPU)
    -> int16 IQ, against the golden vectors of the reference's own code: the same bytes, block for block."""
    pkg.build_frontend()
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    fs, nsamp = float(z["fs"]), int(z["nsamp"])
    blocks = [int(b) for b in z["blocks"]]
    fe = pkg.FrontEnd(os.path.join(GOLDEN, nav), llh=(30.286502, 120.032669, 100.0),
                      motion=os.path.join(GOLDEN, motion) if motion else None, max_chan=max_chan, **kw)
    ch = fe.generate(max(blocks) + 1)
    fe.close()
    b = synth.batch(ch, 1.0 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    want_st = z["end_state"].view(pkg.STATE_DTYPE).reshape(len(blocks), -1)
    for k, blk in enumerate(blocks):
        assert (iq[blk, :z["iq_prefix"].shape[1]] == z["iq_prefix"][k]).all(), (name, blk)
        assert sha(iq[blk]) == str(z["iq_sha256"][k]), (name, blk)
        assert_state_equal(st[blk], want_st[k], ch["prn"][blk] > 0)
    assert synth.hazards(reset=True) == {"itable_512": 0, "dwrd_oob": 0}


def test_feedback_loop_across_a_channel_hand_over(pkg, synth):
    """One gpsbb_fill_block per block with gpsfe_feed_back, across the 30 s maintenance that hands channel 10 from PRN 11
    to PRN 18 in one pass (swap_S): the IQ of the blocks around it equals the reference's, i.e. the new satellite did
    not inherit the old one's carrier phase."""
    pkg.build_frontend()
    z = np.load(os.path.join(GOLDEN, "swap_S.npz"))
    fs, nsamp = float(z["fs"]), int(z["nsamp"])
    blocks = [int(b) for b in z["blocks"]]
    fe = pkg.FrontEnd(os.path.join(GOLDEN, "dense3540.14n"), llh=(30.286502, 120.032669, 100.0), max_chan=16,
                      start=(2014, 12, 20, 1, 20, 0.0))
    for blk in range(max(blocks) + 1):
        ch = fe.next_block()
        iq, st = synth.fill_block(ch, 1.0 / fs, nsamp)
        fe.feed_back(st)
        if blk in blocks:
            assert (iq == z["iq_prefix"][blocks.index(blk)]).all(), blk
    fe.close()


def test_single_block_feedback_loop_like_the_reference(pkg, synth):
    """The drop-in shape: one gpsbb_fill_block per 0.1 s with the carrier phase fed back to the front end,
    as the reference's loop updates chan[] in place; must equal the golden run."""
    pkg.build_frontend()
    z = np.load(os.path.join(GOLDEN, "static_F.npz"))
    fs, nsamp = float(z["fs"]), int(z["nsamp"])
    fe = pkg.FrontEnd(os.path.join(GOLDEN, "synth3540.14n"), llh=(30.286502, 120.032669, 100.0), max_chan=12)
    for blk in range(3):
        ch = fe.next_block()
        iq, st = synth.fill_block(ch, 1.0 / fs, nsamp)
        fe.feed_back(st)
        assert sha(iq) == str(z["iq_sha256"][blk]), blk
    fe.close()


def test_gpsbb_sim_end_to_end_file(pkg, tmp_path):
    """The C program with the reference's structure (front end -> gpsbb_fill_block -> mutex/condvar TX
    surface -> file): its output file must be the golden blocks, byte for byte."""
    import subprocess
    pkg.build_frontend()
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    z = np.load(os.path.join(GOLDEN, "static_F.npz"))
    nsamp = int(z["nsamp"])
    out = str(tmp_path / "iq.bin")
    subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100",
                    "-s", "2600000", "-d", "0.3", "-o", out], check=True, stderr=subprocess.DEVNULL)
    iq = np.fromfile(out, np.int16).reshape(3, nsamp, 2)
    for blk in range(3):
        assert sha(iq[blk]) == str(z["iq_sha256"][blk]), blk
    # (iq_buff is registered with the library by default — gpsbb_host_register: rendered into directly; -R: copied into)
    copied = str(tmp_path / "iq_copied.bin")
    subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100",
                    "-s", "2600000", "-d", "0.3", "-R", "-o", copied], check=True, stderr=subprocess.DEVNULL)
    assert open(copied, "rb").read() == open(out, "rb").read()
    # -F: the same bytes through the streaming ring (front end running ahead, host-chained carrier)
    fast = str(tmp_path / "iq_fast.bin")
    subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100",
                    "-s", "2600000", "-d", "30.1", "-F", "-o", fast], check=True, stderr=subprocess.DEVNULL)
    iq = np.fromfile(fast, np.int16).reshape(301, nsamp, 2)
    for k, blk in enumerate(int(b) for b in z["blocks"]):
        assert sha(iq[blk]) == str(z["iq_sha256"][k]), blk


# ---- GPSBB_FIXED_CARRIER: the reference's `#ifndef FLOAT_CARR_PHASE` carrier NCO -------------------------

def _fixed_desc(pkg, nblocks, nch, seed):
    ch = pkg.synth_descriptors(nblocks, nch=nch, seed=seed)
    ch["carr_phase"] = np.floor(ch["carr_phase"] * 2.0 ** 32)
    return ch


@pytest.mark.parametrize("fs,nsamp,nch,seed", [(25e6, 100000, 16, 201), (2.6e6, 300000, 12, 202), (1e6, 4097, 3, 203)])
def test_fixed_carrier_single_block(pkg, synth, oracle, fs, nsamp, nch, seed):
    ch = _fixed_desc(pkg, 1, nch, seed)[0]
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp, fixed=True)
    iq, st = synth.fill_block(ch, 1.0 / fs, nsamp, flags=pkg.FIXED_CARRIER)
    assert (iq == want_iq[0]).all()
    assert_state_equal(st, want_st[0], ch["prn"] > 0)


@pytest.mark.parametrize("fs,nsamp,nch", [(25e6, 70001, 16), (16.368e6, 50000, 9), (2.6e6, 70001, 12), (4.092e6, 30000, 16)])
def test_fixed_carrier_on_the_model_kernels(pkg, synth, oracle, fs, nsamp, nch, request):
    """The 32-bit accumulator is exactly linear, so the model kernels take it without guard tests on the carrier side
    (k_synth_ev_fixed above ~15.9 MS/s, k_synth_pd below).  Steps that are powers of two put index changes exactly ON
    samples (the tie the 2^-17 in EvConst::tK0 is there for), either sign (a falling phase is mirrored bit by bit), a zero
    step, start phases with all-zero and all-one low halves."""
    ch = _fixed_desc(pkg, 3, nch, 977)
    delt = 1.0 / fs
    rng = np.random.default_rng(5)
    steps = np.array([(1 << int(rng.integers(4, 14))) * (1 if i % 2 else -1) for i in range(nch)], dtype=np.float64)
    steps[0] = 0.0
    steps[1] = 12345.0
    steps[2] = -777.0
    ch["f_carr"] = steps[None, :] / (512.0 * 65536.0 * delt)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    ch["carr_phase"][0, 3:6] = [0.0, 65536.0 * 17, 65536.0 * 400 + 65535.0]
    want_iq, want_st, _ = oracle.fill_blocks(ch, delt, nsamp, chain=True, fixed=True)
    b = synth.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER | pkg.FIXED_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    assert (iq == want_iq).all()
    for k in range(3):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    if "per-sample" not in request.node.callspec.params["seed_mode"]:
        assert synth.info(pkg.INFO_LAST_KERNEL) == 2


def test_fixed_carrier_where_channels_straddle_the_one_chip_per_run_limit(pkg, synth, oracle):
    """fs = 15.5 * 1.023e6: with code Dopplers of both signs some channels hold one chip change per run of 16 samples
    (breakpoint path) and some two (per sample).  The IEEE carrier has a mixed kernel (k_synth_ev_dense); the 32-bit
    accumulator has none, so such a batch must go to the stepped kernel.  Power-of-two steps put index changes exactly on
    samples, falling phases included: what a wrongly chosen IEEE body (mirror 512 - y) would place one sample early."""
    fs, nsamp, nch = 15.8565e6, 60000, 12
    delt = 1.0 / fs
    ch = _fixed_desc(pkg, 2, nch, 4711)
    steps = np.array([(1 << (5 + i % 8)) * (1 if i % 2 else -1) for i in range(nch)], dtype=np.float64)
    steps[3] = -4097.0
    ch["f_carr"] = steps[None, :] / (512.0 * 65536.0 * delt)
    ch["f_code"] = 1.023e6 + np.where(np.arange(nch) % 3 == 0, -40.0, 40.0)[None, :]
    sc = ch["f_code"][0] * delt * 15.5
    assert (sc < 1.0).any() and (sc >= 1.0).any()
    ch["carr_phase"][0, :4] = [0.0, 65536.0 * 511 + 65535.0, 65536.0 * 256, 65535.0]
    for flags_chain in (0, pkg.CHAIN_CARRIER):
        want_iq, want_st, _ = oracle.fill_blocks(ch, delt, nsamp, chain=bool(flags_chain), fixed=True)
        b = synth.batch(ch, delt, nsamp, flags=flags_chain | pkg.FIXED_CARRIER)
        b.run()
        synth.sync()
        iq, st = b.read()
        b.close()
        assert (iq == want_iq).all()
        for k in range(2):
            assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
        assert synth.info(pkg.INFO_LAST_KERNEL) == 1  # the stepped kernel: no mixed model kernel for the accumulator
    # the IEEE carrier on the same rates does have one
    ch2 = pkg.synth_descriptors(2, nch=nch, seed=4712)
    ch2["f_code"] = ch["f_code"]
    want_iq, _, _ = oracle.fill_blocks(ch2, delt, nsamp)
    b = synth.batch(ch2, delt, nsamp)
    b.run()
    synth.sync()
    iq, _ = b.read()
    b.close()
    assert (iq == want_iq).all()


def test_fixed_carrier_chained_batch_and_stream(pkg, synth, oracle):
    ch = _fixed_desc(pkg, 8, 10, 211)
    ch["prn"][5:, 3] = 29
    ch["prn"][2, 6] = 0
    delt, nsamp = 1 / 4.092e6, 60000
    want_iq, want_st, _ = oracle.fill_blocks(ch, delt, nsamp, chain=True, fixed=True)
    b = synth.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER | pkg.FIXED_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    assert (iq == want_iq).all()
    for k in range(8):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    s = synth.stream(10, delt, nsamp, 2, depth=2, flags=pkg.CHAIN_CARRIER | pkg.FIXED_CARRIER)
    got = []
    for k in range(4):
        if s.pending == 2:
            got.append(s.pop())
        s.push(ch[2 * k:2 * k + 2])
    while s.pending:
        got.append(s.pop())
    s.close()
    assert (np.concatenate([g[0] for g in got]) == want_iq).all()


def test_fixed_carrier_golden_and_end_to_end(pkg, synth):
    """Golden vectors of the reference built without FLOAT_CARR_PHASE, from captured descriptors and from
    the RINEX file through the front end."""
    pkg.build_frontend()
    z = np.load(os.path.join(GOLDEN, "static_F_fixed.npz"))
    fs, nsamp = float(z["fs"]), int(z["nsamp"])
    blocks = [int(b) for b in z["blocks"]]
    desc = z["desc"].view(pkg.CHAN_DTYPE).reshape(len(blocks), -1)
    for k in range(len(blocks)):
        iq, _ = synth.fill_block(desc[k], 1.0 / fs, nsamp, flags=pkg.FIXED_CARRIER)
        assert sha(iq) == str(z["iq_sha256"][k]), k
    fe = pkg.FrontEnd(os.path.join(GOLDEN, "synth3540.14n"), llh=(30.286502, 120.032669, 100.0), max_chan=12,
                      fixed_carrier=True)
    ch = fe.generate(3)
    fe.close()
    b = synth.batch(ch, 1.0 / fs, nsamp, flags=pkg.CHAIN_CARRIER | pkg.FIXED_CARRIER)
    b.run()
    synth.sync()
    iq, _ = b.read()
    b.close()
    for blk in range(3):
        assert sha(iq[blk]) == str(z["iq_sha256"][blk]), blk


def test_randomised_shapes_and_dopplers(pkg, synth, oracle):
    """Twenty random workloads: sample rate, block length (odd lengths included), channel count, inactive
    channels, Doppler from mHz to the contract's limit, block count; float and fixed-point carrier;
    independent and chained blocks.  Everything bit-exact against the oracle."""
    rng = np.random.default_rng(20260928)
    for case in range(20):
        fs = float(rng.choice([1e6, 2.6e6, 3e6, 4.092e6, 10e6, 25e6, 30e6]))
        nsamp = int(rng.integers(1, 90000))
        nch = int(rng.integers(1, 17))
        nblocks = int(rng.integers(1, 5))
        fixed = bool(rng.integers(0, 2))
        chain = bool(rng.integers(0, 2))
        ch = pkg.synth_descriptors(nblocks, nch=nch, seed=1000 + case)
        scale = 10.0 ** rng.uniform(-3, np.log10(0.124 * fs), size=(nblocks, nch))
        ch["f_carr"] = np.where(rng.random((nblocks, nch)) < 0.5, -1.0, 1.0) * scale
        ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
        ch["prn"][rng.random((nblocks, nch)) < 0.15] = 0
        if fixed:
            ch["carr_phase"] = np.floor(ch["carr_phase"] * 2.0 ** 32)
        flags = (pkg.FIXED_CARRIER if fixed else 0) | (pkg.CHAIN_CARRIER if chain else 0)
        want_iq, want_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp, chain=chain, fixed=fixed)
        tiles0 = synth.info(pkg.INFO_TILES_RENDERED)
        b = synth.batch(ch, 1.0 / fs, nsamp, flags=flags)
        b.run()
        synth.sync()
        iq, st = b.read()
        b.close()
        what = (case, fs, nsamp, nch, nblocks, fixed, chain)
        assert (iq == want_iq).all(), what
        if synth.info(pkg.INFO_LAST_KERNEL) == 2:  # the model kernels hand tiles out by an atomic they do not wait for: each exactly once
            assert synth.info(pkg.INFO_TILES_RENDERED) - tiles0 == nblocks * ((nsamp + 1023) // 1024), what
        for k in range(nblocks):
            assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    synth.hazards(reset=True)


def test_reference_geometry_runs_on_the_dense_model_kernel(pkg, synth, oracle, request):
    """The reference's own geometry (12 channels, 2.6 MS/s, 300 000-sample blocks, plutogpssim.c:43-45): the table index
    changes at almost every sample there, so every channel is evaluated per sample on the in-tile model
    (k_synth_ev_dense) — chained on the device, bit-exact IQ and end states against the oracle."""
    nb, nch, fs, nsamp = 6, 12, 2.6e6, 300000
    ch = pkg.synth_descriptors(nb, nch=nch, seed=4242)
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    where, kernel = mode_of(request)
    if kernel == "auto":
        assert synth.info(pkg.INFO_LAST_KERNEL) == 2
    for k in range(nb):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    assert (iq == want_iq).all()


def _special_chain_descriptors(pkg, nb, nch, fs, seed):
    """a chained batch with every kind of block the fix-up knows (see test_carrier_chained_on_the_device)"""
    ch = pkg.synth_descriptors(nb, nch=nch, seed=seed)
    rng = np.random.default_rng(seed)
    f0 = rng.uniform(-5000, 5000, nch)
    f0[0], f0[1], f0[2], f0[3] = 3.0, -40.0, 0.0, fs * 2.0 ** -14       # no wrap in a block / none ever / tie-prone step
    ch["f_carr"] = f0[None, :] + rng.uniform(-0.5, 0.5, (nb, nch)) * (np.abs(f0[None, :]) > 100)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    ch["prn"] = np.arange(1, nch + 1)[None, :]
    ch["prn"][nb // 3:, 5] = 31
    ch["prn"][nb // 2:nb // 2 + 3, 9] = 0
    return ch


def test_carrier_chain_alone_on_the_device(pkg, synth, request):
    """gpsbb_chain_carrier: the exact carrier chain on the device with nothing rendered (what seeds a time shard) gives,
    bit for bit, gpsbb_chain_carrier_host's sequential walk — start phase of every block and the phase after the last —
    for special steps (no wrap, ties, idle and re-allocated channels), for the bench's own stream, and for more blocks
    than one sub-batch of the device-side chain takes (the carry crosses sub-batches)."""
    mode = request.node.callspec.params["seed_mode"]
    if not (mode.startswith("k_seed+auto") or mode in ("laps+auto", "default")):  # by the row walks (pass A, prefix, pass B, fix-up) / lap-parallel / the library's choice
        pytest.skip("independent of the other options")
    sys.path.insert(0, ROOT)
    import bench
    cases = [(_special_chain_descriptors(pkg, 700, 16, 25e6, 17), 25e6, 120000),
             (_special_chain_descriptors(pkg, 40, 12, 2.6e6, 18), 2.6e6, 300000),
             (bench.stream_descriptors(pkg, 1500, 16), 25e6, 2500000),
             (bench.stream_descriptors(pkg, 20000, 5, seed=0xC0FFEE), 25e6, 30000)]
    k = np.array([1801439850948, 1801439850949, 3602879701896, 3602879701897, 901439850951, 1201439850950,
                  2201439850947, 1501439850952], dtype=np.float64)
    st = np.concatenate([k[:4] * 2.0 ** -53, k[4:] * 2.0 ** -52, -(2 * k[:4] + 1) * 2.0 ** -54, -k[4:] * 2.0 ** -53])
    tie = pkg.synth_descriptors(600, nch=16, seed=99)
    tie["f_carr"] = (st * 2.0 ** 25)[None, :]
    cases.append((tie, 2.0 ** 25, 300000))
    for ch, fs, nsamp in cases:
        want = pkg.chain_carrier_host(ch, 1 / fs, nsamp)
        got, end = synth.chain_carrier(ch, 1 / fs, nsamp)
        assert got.tobytes() == want.tobytes(), (fs, nsamp, ch.shape)
        # the phase after the last block = where one more block of the same channels would start
        more = np.concatenate([ch, ch[-1:]])
        want_end = pkg.chain_carrier_host(more, 1 / fs, nsamp)[-1]
        assert end.tobytes() == np.where(ch["prn"][-1] > 0, want_end, 0.0).tobytes()
        b0 = ch.shape[0] // 2 + 1
        assert synth.shard_seed(ch, b0, 1 / fs, nsamp).tobytes() == np.where(ch["prn"][b0] > 0, want[b0], ch["carr_phase"][b0]).tobytes()
    with pytest.raises(pkg.GpsbbError):
        bad = cases[0][0][:4].copy()
        bad["f_carr"][2, 1] = np.nan
        synth.chain_carrier(bad, 1 / 25e6, 1000)


def test_options_are_latched_when_a_batch_is_set_up(pkg, synth, oracle, request):
    """A batch keeps the plan it was created with: flipping the handle's options between gpsbb_batch_create and
    gpsbb_batch_run (where the pre-pass runs, where the chain is resolved, which kernel) changes nothing for it."""
    nb, nch, fs, nsamp = 6, 8, 25e6, 60000
    ch = pkg.synth_descriptors(nb, nch=nch, seed=31337)
    ch["f_carr"] = np.linspace(-4000, 4000, nch)[None, :]
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    b = synth.batch(ch, 1 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    saved = []
    try:
        for opt, val in ((pkg.OPT_SEED_WHERE, 2), (pkg.OPT_SEED_WHERE, 1), (pkg.OPT_CHAIN_WHERE, 1), (pkg.OPT_SYNTH_KERNEL, 1)):
            synth.set_option(opt, val)
            b.run()
            synth.sync()
            iq, st = b.read()
            assert (iq == want_iq).all(), (opt, val)
            for k in range(nb):
                assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)
    finally:
        b.close()


def test_stream_changes_sides_between_pushes(pkg, synth, oracle, request):
    """A chained stream whose pushes are resolved now on the device, now on host threads (the handle's options change
    between pushes): the carry moves across and the bytes stay the oracle's."""
    nch, fs, nsamp, bps, npush = 8, 25e6, 50000, 4, 8
    ch = pkg.synth_descriptors(bps * npush, nch=nch, seed=2024)
    ch["f_carr"] = np.linspace(-4500, 4500, nch)[None, :] + np.linspace(0, 3, bps * npush)[:, None]
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / fs, nsamp, chain=True)
    st_ = synth.stream(nch, 1 / fs, nsamp, bps, depth=3, flags=pkg.CHAIN_CARRIER)
    got, gst = [], []
    plan = [(1, 0), (3, 0), (2, 0), (1, 2), (3, 1), (3, 0), (1, 0), (1, 2)]      # (OPT_SEED_WHERE, OPT_CHAIN_WHERE) per push
    for k in range(npush):
        if st_.pending == 3:
            a, b = st_.pop()
            got.append(a), gst.append(b)
        synth.set_option(pkg.OPT_SEED_WHERE, plan[k][0])
        synth.set_option(pkg.OPT_CHAIN_WHERE, plan[k][1])
        st_.push(ch[k * bps:(k + 1) * bps])
    while st_.pending:
        a, b = st_.pop()
        got.append(a), gst.append(b)
    st_.close()
    gst = np.concatenate(gst)
    for k in range(bps * npush):
        assert_state_equal(gst[k], want_st[k], ch["prn"][k] > 0)
    assert (np.concatenate(got) == want_iq).all()



def test_headline_stream_chain_against_the_host_chain(pkg):
    """The bench's own workload: eight pushes of 400 full-size blocks (16 ch, 25 MS/s, 2.5 M samples) of bench.py's
    stream through the HBM-only ring, carrier chained on the device; the end-of-block carrier phases of all 3200
    blocks equal, bit for bit, gpsbb_chain_carrier_host's exact walk of the same descriptors."""
    sys.path.insert(0, ROOT)
    import bench
    PB, nch, delt, nsamp, npush = 400, 16, 1 / 25e6, 2500000, 8
    ch = bench.stream_descriptors(pkg, PB * npush + 1, nch)
    starts = pkg.chain_carrier_host(ch, delt, nsamp)
    with pkg.Synth(0) as s:
        st = s.stream(nch, delt, nsamp, PB, depth=4, flags=pkg.CHAIN_CARRIER | pkg.STREAM_DEVICE_ONLY)
        ends = []
        for k in range(npush):
            if st.pending == 4:
                ends.append(st.pop(copy=False)[1])
            st.push(ch[k * PB:(k + 1) * PB])
        while st.pending:
            ends.append(st.pop(copy=False)[1])
        st.close()
        assert s.info(pkg.INFO_CHAIN_ON_DEVICE) == 1
        assert s.info(pkg.INFO_LAST_KERNEL) == 2
    ends = np.concatenate(ends)["carr_phase"]
    assert ends.tobytes() == starts[1:PB * npush + 1].tobytes()


def test_stream_soak_small(pkg):
    """A slice of the stream soak (tools/fuzz_parity.py --stream): 30 random chained streams — pushes of many short
    blocks through rings of random depth, Dopplers that drift or jump, exact binary steps, channels that change PRN
    or go idle, pre-pass and chain on the device — every one bit-exact against the oracle's sequential render; each also as
    one chained batch and as a batch of independent blocks."""
    import types
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    fuzz_parity.stream_soak(types.SimpleNamespace(cases=30, seed=3, nsamp_max=200000, budget=3e7, ties=False, also_batch=True))


def test_code_rate_soak_small(pkg):
    """A slice of tools/fuzz_parity.py --code-rates: random batches whose channels each have a code rate drawn log-uniformly
    from the whole contract (f_code*delt in [2^-20, 1.5]) and gains whose sum reaches the model kernels' admission limit
    (either sign, some blocks just over it), IEEE and fixed-point carrier, chained or not, every pre-pass and either kernel
    choice: bit-exact against the oracle, the first block also through the drop-in call."""
    import types
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    fuzz_parity.batch_soak(types.SimpleNamespace(cases=40, seed=5, shapes=False, ev=False, only=-1, code_rates=True))


def test_low_rate_soak_with_the_exact_path_forced_often(pkg, request):
    """k_synth_pd's rare path made common: the experiments build with the danger threshold of its models raised from 24 to
    2^22 units of 2^-32 (one test in a thousand instead of one in 10^8 sends a lane to pd_fix_sample: most wavefronts
    then hold lanes that take the model's 16 contributions of a channel out and put exact ones in), over random chained
    streams at 1 .. 10 MS/s with 1 to 16 channels (both chip-table layouts, data bits that change inside tiles)."""
    if request.node.callspec.params["seed_mode"] != ONCE:
        pytest.skip("a process of its own with its own options: once")
    import subprocess
    for where in ("3", "1"):   # on the lap-parallel pre-pass (the product's default) and on the row walks
        env = dict(os.environ, GPSBB_PY_LIB="exp", GPSBB_PD_DANGER=str(1 << 22), GPSBB_FUZZ_WHERE=where)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "--stream", "--low-rate", "--cases", "24",
                            "--seed", "77", "--budget", "1.5e7"], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "bit-exact" in r.stdout


def test_high_rate_soak_with_the_exact_path_forced_often(pkg, request):
    """The same for k_synth_ev: the danger threshold of every channel raised to 2^22 units of 2^-32, so that about one
    lane-run in two hundred is recomputed by ev_exact_run (out of line) — with one or two channels per block the call
    then comes right after the wavefront has claimed its next chunk of tiles, which must not get lost."""
    if request.node.callspec.params["seed_mode"] != ONCE:
        pytest.skip("a process of its own with its own options: once")
    import subprocess
    for where in ("3", "1"):   # on the lap-parallel pre-pass (the product's default) and on the row walks
        env = dict(os.environ, GPSBB_PY_LIB="exp", GPSBB_EV_DANGER=str(1 << 22), GPSBB_FUZZ_WHERE=where)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "--stream", "--cases", "30", "--seed", "78",
                            "--budget", "1.5e7"], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "bit-exact" in r.stdout


GRAZE_OFFSETS = [0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6, 8, -8, 10, -10, 12, -12, 13, -13, 14, -14, 16, -16, 20, -20, 24, -24,
                 28, -28, 32, -32, 48, -48]


@pytest.mark.parametrize("fs,nch,nsamp,dopp,fixed,samples", [
    (25e6, 16, 100000, 5000.0, False, None),                                      # k_synth_ev
    (25e6, 16, 70001, 12000.0, False, [16, 15, 1008, 1023, 1024, 1025, 2047, 70000, 69985, 5000, 777]),
    (16.0e6, 16, 60000, 3000.0, False, None),                                     # ... at its one-chip-per-run limit
    (15.8565e6, 12, 60000, 5000.0, False, None),                                  # k_synth_ev_dense (mixed)
    (25e6, 16, 100000, 5000.0, True, None),                                       # k_synth_ev_fixed (code NCO)
    (2.6e6, 12, 100000, 20000.0, False, None),                                    # k_synth_pd, two chip tables
    (2.6e6, 16, 100000, 300000.0, False, [64, 63, 960, 1023, 1024, 1087, 99999, 99936, 4097]),  # ... one table, fast carriers
    (3.0e6, 12, 60000, 5000.0, True, None),                                       # k_synth_pd, the accumulator (code NCO)
])
def test_states_that_graze_an_integer_at_a_sample(pkg, synth, oracle, fs, nch, nsamp, dopp, fixed, samples):
    """The adversarial case of the model kernels: descriptors aimed so that the REFERENCE's carrier phase * 512 (c:2697)
    or code phase (c:2737) is within 0, +-1, +-2 ... +-48 units of 2^-32 of an integer exactly at a sample — either side
    of it, inside the kernels' danger band (exact path) and just outside it (the model is trusted) — at run starts, run
    ends, tile edges and the block's last sample.  Everything bit-exact against the oracle, in every mode."""
    graze(pkg, synth, oracle, fs, nch, nsamp, dopp, fixed, samples)


def graze(pkg, synth, oracle, fs, nch, nsamp, dopp, fixed, samples, f_code=None):
    nb = 5
    ch, targets = pkg.grazing_descriptors(nb, nch, fs, nsamp, GRAZE_OFFSETS, seed=int(fs) % 1000 + nch, max_doppler=dopp,
                                          fixed=fixed, samples=samples, f_code=f_code)
    assert all(abs(t[5] - t[4]) <= 0.3 for t in targets), "the generator missed a target"
    flags = pkg.FIXED_CARRIER if fixed else 0
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp, fixed=fixed)
    b = synth.batch(ch, 1.0 / fs, nsamp, flags=flags)
    b.run()
    synth.sync()
    iq, st = b.read()
    b.close()
    assert (iq == want_iq).all()
    for k in range(nb):
        assert_state_equal(st[k], want_st[k], ch["prn"][k] > 0)


# the products f_code*delt ev_plan decides on (tests/contract_corners.py): the floor of the model kernels, a slow code, either
# side of one chip change per run, and the last product the chip table reaches
GRAZE_SC = {"2^-20": 2.0 ** -20, "1e-4": 1e-4, "1/15.5-": float(np.nextafter(1 / 15.5, 0.0)),
            "1/15.5+": float(np.nextafter(np.nextafter(1 / 15.5, 1.0), 1.0)), "0.5": 0.5, "543/1040-": 543.0 / 1040.0 - 2.0 ** -45}


@pytest.mark.parametrize("fs,nch,nsamp,dopp,fixed,samples,sc", [
    (25e6, 16, 70001, 5000.0, False, None, "2^-20"),                              # k_synth_ev, rsc = 2^20
    (25e6, 16, 70001, 5000.0, False, [16, 15, 1008, 1023, 1024, 1025, 2047, 70000, 69985, 5000, 777], "1e-4"),
    (25e6, 16, 70001, 5000.0, False, None, "1/15.5-"),                            # ... its last product
    (25e6, 16, 70001, 5000.0, True, None, "1/15.5-"),                             # k_synth_ev_fixed there
    (25e6, 12, 70001, 5000.0, False, None, "1/15.5+"),                            # k_synth_pd at 25 MS/s: its first product
    (25e6, 16, 70001, 5000.0, False, None, "0.5"),
    (25e6, 12, 70001, 5000.0, False, [64, 63, 960, 1023, 1024, 1087, 70000, 69937, 4097], "543/1040-"),   # the chip table's reach
    (25e6, 16, 70001, 5000.0, True, None, "543/1040-"),
    (2.6e6, 12, 70001, 20000.0, False, None, "1/15.5+"),
    (2.6e6, 16, 70001, 20000.0, False, None, "0.5"),
    (2.6e6, 12, 70001, 20000.0, False, [64, 63, 960, 1023, 1024, 1087, 70000, 69937, 4097], "543/1040-"),
    (2.6e6, 16, 70001, 5000.0, True, None, "543/1040-"),
    (1e6, 16, 70001, 5000.0, False, None, "2^-20"),                               # k_synth_ev_dense: slow code, fast carriers
])
def test_code_rates_that_graze_an_integer_at_a_sample(pkg, synth, oracle, fs, nch, nsamp, dopp, fixed, samples, sc):
    """test_states_that_graze_an_integer_at_a_sample along the code-rate axis: every channel at one of the products
    f_code*delt the planner decides on, reached exactly, with the code NCO (and the carrier, as there) aimed at integers."""
    f_code = pkg.code_rate_for(GRAZE_SC[sc], fs)
    assert f_code is not None and f_code * (1.0 / fs) == GRAZE_SC[sc]
    graze(pkg, synth, oracle, fs, nch, nsamp, dopp, fixed, samples, f_code=f_code)


def test_the_failure_the_round_3_budgets_allowed(pkg, synth, oracle, request):
    """tests/golden/graze_r3_fail.npz: blocks found by tools/graze_hunt.py in which the library built with the error
    budgets of rounds 2-3 (make r3budgets) places a chip or table-index change one sample late — the truth lands a
    fraction of a unit of 2^-32 above an integer at a sample while the lane's first-sample model, roundings of the guard
    format included, sits more than W * step below it: outside the band the danger test covered.  The
    product renders every one of them bit-exactly, in every mode; the old budgets still fail them (which is what makes
    this a test of the budgets and not of luck)."""
    z = np.load(os.path.join(GOLDEN, "graze_r3_fail.npz"))
    nsamp = int(z["nsamp"])
    names = [k[5:] for k in z.files if k.startswith("desc_")]
    assert names
    for name in names:
        fs = float(z["fs_" + name])
        ch = z["desc_" + name].view(pkg.CHAN_DTYPE).reshape(-1, int(z["nch_" + name]))
        want_iq, _, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
        b = synth.batch(ch, 1.0 / fs, nsamp)
        b.run()
        synth.sync()
        iq, _ = b.read()
        b.close()
        assert (iq == want_iq).all(), name
    if request.node.callspec.params["seed_mode"] != ONCE:
        return
    import json
    import subprocess
    import tempfile
    vdir = tempfile.mkdtemp(prefix="gpsbb_variants_")  # (never beside the product: csrc/Makefile)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "pluto-gps-sim_amd", "csrc"), "r3budgets", "VARIANT_DIR=" + vdir])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "graze_hunt.py"), "--load", os.path.join(GOLDEN, "graze_r3_fail.npz")],
                       env=dict(os.environ, GPSBB_PY_LIB=os.path.join(vdir, "libgpsbb_r3budgets.so")), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["lib"] == "libgpsbb_r3budgets.so"
    assert sum(c["mismatching_samples"] for c in doc["cases"].values()) >= len(names), doc


def test_model_error_budgets_are_measured_not_summed(pkg, request):
    """The bit-exactness of k_synth_ev / k_synth_pd rests on |in-tile model - reference recurrence| <= W (EvConst::W,
    PD_BAND).  tools/model_err.py replays, on the experiments build of the same sources, the fast paths' own arithmetic
    next to the reference's recurrence stepped sample by sample for every tile of 31 workloads at the corners of what
    the kernels take (gpsbb_modelerr.hip.h).  Asserted: no unflagged decision differs from the truth; the replay flags
    exactly the lane-runs the kernel itself sent to the exact path; the realised error of everything tested is at most HALF
    its budget; the plain linear model stays within the derived 2^-33.9 (0.27 units; EV_MODEL_ERR allows 1)."""
    if request.node.callspec.params["seed_mode"] != ONCE:
        pytest.skip("a process of its own with its own options: once")
    import json
    import subprocess
    env = dict(os.environ, GPSBB_PY_LIB="exp")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "model_err.py"), "--quick"], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "MODEL_ERR_DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    doc = json.loads(r.stdout[:r.stdout.rindex("MODEL_ERR_DONE")])
    for name, w in doc["workloads"].items():
        assert "max" in w, (name, w)
        assert w["bad_unflagged_decisions"] == 0, (name, w)
        assert w["lanes_flagged"] + w["always_exact"] == w["kernel_exact_runs"], (name, w)
        assert w.get("iq_mismatches_vs_oracle", 0) == 0, (name, w)
        for q in ("y0_over_W", "tk_over_W", "x0_over_W", "tc_over_W"):
            assert w["max"][q] <= 0.5, (name, q, w["max"])
        assert w["max"]["pure_y"] <= 0.27 and w["max"]["pure_x"] <= 0.27, (name, w["max"])


def test_time_shards_through_the_ring_give_one_digest(pkg, synth, oracle):
    """BASELINE configs[4] in small: a stream continuous in time (drifting Dopplers, carrier carried from block
    to block) cut into 1, 2 and 3 contiguous time shards; each shard is rendered on its own through the
    streaming ring from the exact carrier seed of its first block.  The per-block digests must equal the
    oracle's render of the whole stream, whatever the number of shards and the slot size."""
    import hashlib
    import importlib.util
    spec = importlib.util.spec_from_file_location("shard_stream", os.path.join(os.path.dirname(GOLDEN), "..", "tools",
                                                                               "shard_stream.py"))
    ss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ss)
    fs, nsamp, nblocks, nch = 25e6, 50000, 13, 16
    delt = 1.0 / fs
    ch = ss.stream_descriptors(pkg, nblocks, nch, seed=0xABCD)
    ch["prn"][7:, 3] = 21                       # a channel re-allocated to another satellite: its phase restarts
    want_iq, _, _ = oracle.fill_blocks(ch, delt, nsamp, chain=True)
    want = [hashlib.sha256(want_iq[k].tobytes()).digest() for k in range(nblocks)]
    seeds = pkg.chain_carrier_host(ch, delt, nsamp)
    for world, bps in ((1, 4), (2, 3), (3, 2)):
        got = []
        for rank in range(world):
            b0, b1 = pkg.shard_blocks(nblocks, rank, world)
            d, _ = ss.shard_digests(pkg, synth, ch, seeds, b0, b1, delt, nsamp, bps)
            got += d
        assert got == want, (world, bps)



def test_config5_at_full_block_size_in_1_2_and_4_time_shards(pkg, synth, oracle, request):
    """BASELINE configs[4] at its real block size: 360 s of the 16-channel 25 MS/s stream (3600 blocks of 2.5 M samples,
    9e9 samples, 36 GB) through the ring with the pinned gather, on one GPU, as 1, 2 and 4 contiguous time shards.  A
    shard starts from the stream's exact carrier phase there (gpsbb_chain_carrier_host) and chains on the device from
    then on; every block is digested as it lands in pinned host memory.  The digest of the block digests must not
    depend on the number of shards, two blocks are compared with the CPU oracle in full, and no hazard may have
    been counted.  (Run once, with no option set — the lap-parallel pre-pass, what the product runs; the forced variants are covered at small sizes.)"""
    if request.node.callspec.params["seed_mode"] != ONCE:
        pytest.skip("full-size run: once")
    import xxhash
    import bench
    nch, fs, nsamp, nb, bps, depth = 16, 25e6, 2500000, 3600, 36, 4
    delt = 1.0 / fs
    ch = bench.stream_descriptors(pkg, nb, nch)
    seeds = pkg.chain_carrier_host(ch, delt, nsamp)
    synth.hazards(reset=True)

    def render(nshards):
        digs = []
        for r in range(nshards):
            b0, b1 = pkg.shard_blocks(nb, r, nshards)
            mine = ch[b0:b1].copy()
            mine["carr_phase"][0] = seeds[b0]
            st = synth.stream(nch, delt, nsamp, bps, depth=depth, flags=pkg.CHAIN_CARRIER)
            nslots = (b1 - b0) // bps
            pushed = popped = 0
            while popped < nslots:
                while pushed < nslots and st.pending < depth:
                    st.push(mine[pushed * bps:(pushed + 1) * bps])
                    pushed += 1
                iq, _ = st.pop(copy=False)
                digs.extend(xxhash.xxh3_64_intdigest(memoryview(iq[k]).cast("B")) for k in range(bps))
                popped += 1
            st.close()
        return digs

    one = render(1)
    assert synth.info(pkg.INFO_CHAIN_ON_DEVICE) == 1 and synth.info(pkg.INFO_LAST_KERNEL) == 2
    assert synth.info(pkg.INFO_PREPASS) == 3   # no option set: the lap-parallel pre-pass, what the product runs
    assert len(one) == nb
    for n in (2, 4):
        assert render(n) == one, "%d shards" % n
    assert synth.hazards(reset=True) == {"itable_512": 0, "dwrd_oob": 0}
    # two blocks in full against the CPU oracle, started from the host chain's exact phase
    for b in (2700, 3599):
        d = ch[b:b + 1].copy()
        d["carr_phase"][0] = seeds[b]
        want, _, _ = oracle.fill_blocks(d, delt, nsamp)
        assert xxhash.xxh3_64_intdigest(memoryview(np.ascontiguousarray(want[0])).cast("B")) == one[b], b


def test_config5_at_its_stated_length(pkg, synth, oracle, request):
    """BASELINE configs[4] at its STATED length: 3600 s of the 16-channel 25 MS/s stream — 36 000 blocks of 2.5 M samples,
    9e10 samples, 360 GB of int16 IQ — chained on the device and gathered into pinned host memory through the ring on one
    GPU, every block digested (xxh3) as it lands.  The carrier phase at the end of every one of the 36 000 blocks equals
    gpsbb_chain_carrier_host's sequential walk bit for bit; the digests of the first 3600 blocks equal those of the same
    descriptors rendered as a stream of their own; two blocks from the stream's far end equal the CPU oracle's render from
    the phase the stream reports there; no hazard.  The sustained gather rate goes to gpurun_out/ (copied to profiles/)."""
    if request.node.callspec.params["seed_mode"] != ONCE:
        pytest.skip("full-length run: once")
    import json
    import time
    from concurrent.futures import ThreadPoolExecutor
    import xxhash
    import bench
    nch, fs, nsamp, nb, bps, depth = 16, 25e6, 2500000, 36000, 36, 6
    delt = 1.0 / fs
    ch = bench.stream_descriptors(pkg, nb, nch)
    synth.hazards(reset=True)
    pool = ThreadPoolExecutor(8)

    def render(nblocks):
        digs, ends, pend = [None] * nblocks, [], {}
        st = synth.stream(nch, delt, nsamp, bps, depth=depth, flags=pkg.CHAIN_CARRIER)
        nslots = nblocks // bps
        pushed = popped = 0
        t0 = time.perf_counter()
        while popped < nslots:
            while pushed < nslots and st.pending < depth:
                for f in pend.pop(pushed % depth, []):     # the slot's previous blocks have been digested
                    f.result()
                st.push(ch[pushed * bps:(pushed + 1) * bps])
                pushed += 1
            iq, e = st.pop(copy=False)
            ends.append(e["carr_phase"].copy())

            def job(k, v):
                digs[k] = xxhash.xxh3_64_intdigest(v)
            pend[popped % depth] = [pool.submit(job, popped * bps + k, memoryview(iq[k]).cast("B")) for k in range(bps)]
            popped += 1
        for fs_ in pend.values():
            for f in fs_:
                f.result()
        dt = time.perf_counter() - t0
        st.close()
        return digs, np.concatenate(ends), dt

    digs, ends, dt = render(nb)
    assert synth.info(pkg.INFO_CHAIN_ON_DEVICE) == 1 and synth.info(pkg.INFO_LAST_KERNEL) == 2
    assert synth.info(pkg.INFO_PREPASS) == 3   # no option set: the lap-parallel pre-pass, what the product runs
    assert synth.hazards(reset=True) == {"itable_512": 0, "dwrd_oob": 0}
    starts = pkg.chain_carrier_host(np.concatenate([ch, ch[-1:]]), delt, nsamp)
    assert ends.tobytes() == starts[1:].tobytes()                      # all 36 000 end-of-block carrier phases
    first, _, _ = render(3600)
    assert first == digs[:3600]
    # the far end against the oracle: blocks nb-2, nb-1 from the phase the stream reports at the end of block nb-3
    tail = ch[nb - 2:].copy()
    tail["carr_phase"][0] = ends[nb - 3]
    want_iq, want_st, _ = oracle.fill_blocks(tail, delt, nsamp, chain=True)
    assert [xxhash.xxh3_64_intdigest(want_iq[k].tobytes()) for k in range(2)] == digs[nb - 2:]
    assert want_st["carr_phase"].tobytes() == ends[nb - 2:].tobytes()
    rec = {"blocks": nb, "samples": nb * nsamp, "iq_bytes": nb * nsamp * 4, "seconds": dt, "GB_per_s_to_pinned_host": nb * nsamp * 4 / dt / 1e9,
           "samples_per_s": nb * nsamp / dt, "ring": {"slot_blocks": bps, "depth": depth},
           "digest_of_block_digests": "%016x" % xxhash.xxh3_64_intdigest(np.asarray(digs, np.uint64).tobytes()),
           "checks": "36000 end-of-block carrier phases == gpsbb_chain_carrier_host; first 3600 block digests == the same descriptors as a "
                     "stream of their own; last two blocks == CPU oracle; hazards zero"}
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):
        json.dump(rec, open(os.path.join(out, "config5_full.json"), "w"), indent=1)
    print(json.dumps(rec))


def test_handle_and_batch_lifecycle(pkg, oracle):
    """Create/destroy churn, one handle reused across shapes, many small blocks in one batch, API misuse."""
    import ctypes as C
    for _ in range(3):
        with pkg.Synth(0) as s:
            for nch, nsamp, nblocks in [(3, 1000, 1), (16, 5000, 7), (1, 17, 2), (12, 300000, 1)]:
                ch = pkg.synth_descriptors(nblocks, nch=nch, seed=nch * 7 + nblocks)
                want, _, _ = oracle.fill_blocks(ch, 1 / 4.092e6, nsamp)
                b = s.batch(ch, 1 / 4.092e6, nsamp)
                b.run()
                s.sync()
                assert (b.read()[0] == want).all()
                b.close()
                iq, _ = s.fill_block(ch[0], 1 / 4.092e6, nsamp)   # the scratch batch grows and shrinks with the call
                assert (iq == want[0]).all()
    with pkg.Synth(0) as s:
        ch = pkg.synth_descriptors(3000, nch=4, seed=5)           # many short blocks, chained on the host
        want, want_st, _ = oracle.fill_blocks(ch, 1 / 2.6e6, 2000, chain=True)
        b = s.batch(ch, 1 / 2.6e6, 2000, flags=pkg.CHAIN_CARRIER)
        b.run()
        s.sync()
        iq, st = b.read()
        assert (iq == want).all() and st["carr_phase"].tobytes() == want_st["carr_phase"].tobytes()
        b.close()
        L = pkg.lib()
        h = s._h
        one = pkg.synth_descriptors(1, nch=2, seed=1)
        out = C.c_void_p()
        assert L.gpsbb_batch_create(h, one.ctypes.data, 0, 2, 1e-6, 10, 0, C.byref(out)) == -1      # nblocks < 1
        assert L.gpsbb_batch_create(h, one.ctypes.data, 1, 17, 1e-6, 10, 0, C.byref(out)) == -1     # nch > 16
        assert L.gpsbb_batch_create(h, one.ctypes.data, 1, 2, 1e-6, 10, 8, C.byref(out)) == -1      # unknown flag
        assert L.gpsbb_batch_create(h, one.ctypes.data, 1, 2, -1.0, 10, 0, C.byref(out)) == -1      # delt <= 0
        assert L.gpsbb_batch_read(None, None, None) == -7
        st = s.stream(2, 1e-6, 100, 1, depth=2)
        with pytest.raises(pkg.GpsbbError) as e:
            st.pop()                                              # nothing pushed
        assert e.value.rc == -7
        st.close()
