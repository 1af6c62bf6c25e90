"""Multipath echoes in the host front end (include/gpsfe.h gpsfe_set_echoes): an echo is a channel of its own in the reference's
arithmetic — its satellite's PRN and data words, the code phase and bit counters of a longer range, a carrier phase of its own, a
scaled gain — in slot max_chan + j, which channel allocation never sees.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

SITE = (30.286502, 120.032669, 100.0)
C_LIGHT = 2.99792458e8
LAMBDA = C_LIGHT / 1575.42e6
# tests/test_frontend.py's hand-over scenario with 12 channels: the maintenance of block 1499 frees slot 10 (PRN 11 has set) and
# gives it to PRN 13 in the same pass
SWAP = dict(nav="dense3540.14n", start=(2014, 12, 20, 1, 20, 0.0))
ECHOES = [(11, 100.0, 6.0), (13, 350.0, 3.0, 0.25, 1.5), (5, 29000.0, 10.0, 0.5, -2.0), (5, 12.5, 1.0)]


@pytest.fixture(scope="module")
def fe_pkg(pkg):
    pkg.build_frontend()
    return pkg


def front_end(pkg, nav="synth3540.14n", max_chan=12, echoes=None, threads=None, **kw):
    fe = pkg.FrontEnd(os.path.join(GOLDEN, nav), llh=SITE, max_chan=max_chan, **kw)
    if echoes is not None:
        fe.set_echoes(echoes)
    if threads is not None:
        fe.set_threads(threads)
    return fe


def test_without_echoes_nothing_changes_and_the_satellites_slots_never_do(fe_pkg):
    """No echoes set: gpsfe_next_block gives what the reference's dumps hold (tests/golden/static_F.npz, which the parent commit
    reproduces: tests/test_frontend.py) — at the blocks the dump sampled, in every field but carr_phase, which the reference
    carries in its sample loop.  That is the only comparison with anything outside this code.  The rest compares the code with
    itself, which pins the paths against each other and not against the parent: gpsfe_generate on 1 and on 5 threads, with no
    call to gpsfe_set_echoes and with a call that sets none, against those blocks across the maintenances of blocks 299 and
    599; and with echoes set, slots 0 .. max_chan-1 against the same bytes, again on every path."""
    pkg = fe_pkg
    n = 620
    fe = front_end(pkg)
    want = np.stack([fe.next_block() for _ in range(n)])
    assert fe.block_chans == 12
    fe.close()
    z = np.load(os.path.join(GOLDEN, "static_F.npz"))
    ref = z["desc"].view(pkg.CHAN_DTYPE).reshape(len(z["blocks"]), -1)
    for k, b in enumerate(int(v) for v in z["blocks"]):
        if b < n:
            for f in ("prn", "iword", "ibit", "icode", "f_carr", "f_code", "code_phase", "gain", "dwrd"):
                assert np.ascontiguousarray(want[b][f]).tobytes() == np.ascontiguousarray(ref[k][f]).tobytes(), (b, f)
    for echoes in (None, []):
        for threads in (1, 5):
            fe = front_end(pkg, echoes=echoes, threads=threads)
            assert fe.generate(n).tobytes() == want.tobytes(), (echoes, threads)
            fe.close()
    prns = [int(p) for p in want["prn"][0] if p > 0]
    echoes = [(prns[0], 75.0, 6.0), (prns[3], 1000.0, 3.0, 0.3, 2.0), (prns[0], 0.0, 0.0)]
    for threads in (1, 5):
        fe = front_end(pkg, echoes=echoes, threads=threads)
        assert fe.block_chans == 15 and fe.max_chan == 12
        got = fe.generate(n)
        fe.close()
        assert got.shape == (n, 15) and np.ascontiguousarray(got[:, :12]).tobytes() == want.tobytes(), threads
    fe = front_end(pkg, echoes=echoes)
    got = np.stack([fe.next_block() for _ in range(n)])
    fe.close()
    assert np.ascontiguousarray(got[:, :12]).tobytes() == want.tobytes()


@pytest.mark.parametrize("fixed", [False, True])
def test_the_null_echo_is_its_direct_channel(fe_pkg, fixed):
    """{prn, 0, 0, 0, 0}: every byte of the echo's descriptor is its direct channel's, in every block, on both carrier variants,
    across the hand-over (PRN 11 sets after block 1499, PRN 13 rises then): while the PRN holds no channel the echo's slot is
    a free slot (prn 0, all zeros)."""
    pkg = fe_pkg
    fe = front_end(pkg, max_chan=12, echoes=[(11, 0.0, 0.0), (13, 0.0, 0.0)], fixed_carrier=fixed, **SWAP)
    ch = fe.generate(1510)
    fe.close()
    seen = {11: [0, 0], 13: [0, 0]}
    for b in range(ch.shape[0]):
        for j, prn in ((12, 11), (13, 13)):
            where = np.flatnonzero(ch["prn"][b, :12] == prn)
            if where.size:
                assert ch[b, j].tobytes() == ch[b, where[0]].tobytes(), (b, prn)
            else:
                assert ch[b, j].tobytes() == bytes(ch.dtype.itemsize), (b, prn)
            seen[prn][int(where.size > 0)] += 1
    assert seen == {11: [10, 1500], 13: [1500, 10]}


def test_generate_equals_next_block_with_echoes(fe_pkg):
    """gpsfe_generate on threads against repeated gpsfe_next_block, byte for byte, with echoes that drift (rate_mps != 0), two
    of one PRN, one that is freed and one that is born at the hand-over; the calls mixed as well."""
    pkg = fe_pkg
    n = 1650
    fe = front_end(pkg, echoes=ECHOES, **SWAP)
    want = np.stack([fe.next_block() for _ in range(n)])
    fe.close()
    assert want.shape == (n, 16)
    assert (want["prn"][1499, 12:] == (11, 0, 5, 5)).all() and (want["prn"][1500, 12:] == (0, 13, 5, 5)).all()
    for threads in (1, 2, 7):
        fe = front_end(pkg, echoes=ECHOES, threads=threads, **SWAP)
        assert fe.generate(n).tobytes() == want.tobytes(), threads
        fe.close()
    fe = front_end(pkg, echoes=ECHOES, threads=5, **SWAP)
    parts = [fe.generate(100), np.stack([fe.next_block() for _ in range(3)]), fe.generate(1297), fe.generate(150), fe.generate(100)]
    fe.close()
    assert np.concatenate(parts).tobytes() == want.tobytes()


def test_feed_back_reads_the_echoes_end_states(fe_pkg):
    """gpsfe_feed_back takes gpsfe_block_chans() end states: an echo's slot keeps what was fed back; what is fed back for a
    slot that was idle in the block is ignored, and the slot stays free"""
    pkg = fe_pkg
    fe = front_end(pkg, echoes=[(11, 100.0, 6.0), (13, 350.0, 3.0)], **SWAP)
    ch = fe.next_block()
    st = np.zeros(14, pkg.STATE_DTYPE)
    st["carr_phase"] = 0.125 + np.arange(14) / 64.0
    st["dataBit"] = 1
    fe.feed_back(st)
    nxt = fe.next_block()
    fe.close()
    assert ch["prn"][12] == 11 and ch["prn"][13] == 0
    assert nxt["carr_phase"][12] == st["carr_phase"][12] and nxt["carr_phase"][0] == st["carr_phase"][0]
    assert nxt["prn"][12] == 11 and nxt[13].tobytes() == bytes(nxt.dtype.itemsize)


def total_chips(d):
    return ((d["iword"].astype(np.float64) * 30 + d["ibit"]) * 20 + d["icode"]) * 1023.0 + d["code_phase"]


def test_an_echo_is_later_weaker_and_shifted_in_doppler(fe_pkg):
    """The three physical statements, each on every block of 40 s around the hand-over and every echo of ECHOES.

    Code phase.  computeCodePhase (c:1754-1787) turns the transmit time t - range / c into milliseconds and those into chips at
    1023 chips per millisecond — the nominal rate, not the Doppler-shifted f_code (they differ by up to 3e-6, which at 29 km is
    3e-4 chips) — so with the counters folded in (((iword * 30 + ibit) * 20 + icode) * 1023 + code_phase) the direct channel
    is ahead of the echo by e(k) / c * 1.023e6 chips.  Roundings: the time difference (below 36 s) is rounded to 2^-48 s, its
    product with 1000 (below 36 000 ms) to 2^-38 ms, range / c to 2^-57 s, range + e (below 2^25 m) to 2^-29 m or 6e-18 s: under
    1.1e-11 ms = 1.2e-8 chips per channel, and folding the counters back in (a number below 3.7e7 chips, rounded to 2^-28) adds
    3.7e-9 each: the difference of two channels is within 3.2e-8 chips, inside the 1e-6 asked for.
    Carrier.  f_carr = -(range(k+1) - range(k)) / 0.1 / lambda on ranges that each carry one more rounding (range + e, half
    an ulp of a number below 2^25 m: 1.9e-9 m): the echo's f_carr is the direct channel's - rate_mps / lambda to
    2 * 1.9e-9 / 0.1 / 0.1903 = 2.0e-7 Hz, plus e(k+1) - e(k) against rate * 0.1 (products below 2^13 m rounded to 2^-41 m:
    nothing), inside 1e-6 Hz.
    Gain.  (g * p) / g with p = 10^(-atten / 20): the product is rounded once and the quotient once, half an ulp each."""
    pkg = fe_pkg
    fe = front_end(pkg, echoes=ECHOES, **SWAP)
    ch = fe.generate(1700)[1300:]   # 40 s around the hand-over of block 1500
    fe.close()
    worst = [0.0, 0.0]
    for j, e in enumerate(ECHOES):
        prn, extra, atten = e[0], e[1], e[2]
        rate = e[4] if len(e) > 4 else 0.0
        for b in range(ch.shape[0]):
            where = np.flatnonzero(ch["prn"][b, :12] == prn)
            if not where.size:   # (PRN 11 has set / PRN 13 has not risen)
                assert ch["prn"][b, 12 + j] == 0
                continue
            d, r = ch[b, int(where[0])], ch[b, 12 + j]
            assert r["prn"] == prn and r["dwrd"].tobytes() == d["dwrd"].tobytes()
            ek = extra + rate * ((1300 + b) / 10.0)
            dchips = (total_chips(d) - total_chips(r)) - ek / C_LIGHT * 1.023e6
            dcarr = (r["f_carr"] - d["f_carr"]) - (-rate / LAMBDA)
            worst = [max(worst[0], abs(dchips)), max(worst[1], abs(dcarr))]
            assert abs(dchips) <= 1e-6, (j, b, dchips)
            assert abs(dcarr) <= 1e-6, (j, b, dcarr)
            assert r["f_code"] == 1.023e6 + r["f_carr"] * (1.0 / 1540.0)
            p = 10.0 ** (-atten / 20.0)
            assert abs(r["gain"] / d["gain"] - p) <= np.spacing(p), (j, b)
    print("worst code-phase error %.3g chips, worst f_carr error %.3g Hz" % tuple(worst))


def test_birth_phase_of_an_echo(fe_pkg):
    """At birth the echo's carrier phase is the direct channel's with the extra path taken off and the reflection added:
    frac((2 r_ref - (r_xyz + e)) / lambda + phase_cyc).  Against the direct channel's frac((2 r_ref - r_xyz) / lambda) that is
    -e / lambda + phase_cyc modulo 1; the two phases are fractions of numbers below 2^28 cycles (ulp 2^-24): 1e-6 covers the
    three roundings.  Checked for the echo born with the scenario and for the one born at the hand-over (e taken at block 1500)."""
    pkg = fe_pkg
    fe = front_end(pkg, echoes=ECHOES, **SWAP)
    ch = fe.generate(1501)
    fe.close()
    for b, j in ((0, 0), (1500, 1), (0, 2)):
        e = ECHOES[j]
        rate = e[4] if len(e) > 4 else 0.0
        cyc = e[3] if len(e) > 3 else 0.0
        i = int(np.flatnonzero(ch["prn"][b, :12] == e[0])[0])
        want = -(e[1] + rate * (b / 10.0)) / LAMBDA + cyc
        diff = (ch["carr_phase"][b, 12 + j] - ch["carr_phase"][b, i] - want) % 1.0
        assert min(diff, 1.0 - diff) < 1e-6, (b, j, diff)


def test_the_oracle_renders_an_echo_as_one_more_channel(fe_pkg, oracle):
    """The reference truncates per channel and adds (the render is sum_i trunc(gain_i * r_i) in int16 arithmetic), so the render
    of the blocks with their echo channels is the render without them plus the render of the echo channels alone, sample for
    sample: an echo really is just a channel, and one PRN in two slots of a block is nothing special."""
    pkg = fe_pkg
    fs, nsamp = 2.6e6, 3 * 1024 + 37
    fe = front_end(pkg, echoes=ECHOES, **SWAP)
    ch = fe.generate(3)
    fe.close()
    assert (ch["prn"][:, 12:] == (11, 0, 5, 5)).all()
    direct, echo = ch.copy(), ch.copy()
    direct["prn"][:, 12:] = 0
    echo["prn"][:, :12] = 0
    both = oracle.fill_blocks(ch, 1.0 / fs, nsamp, chain=True)[0]
    a = oracle.fill_blocks(direct, 1.0 / fs, nsamp, chain=True)[0]
    b = oracle.fill_blocks(echo, 1.0 / fs, nsamp, chain=True)[0]
    assert np.abs(b).max() > 0
    assert (both == (a.astype(np.int32) + b.astype(np.int32)).astype(np.int16)).all()
    assert (a == oracle.fill_blocks(np.ascontiguousarray(ch[:, :12]), 1.0 / fs, nsamp, chain=True)[0]).all()


def test_set_echoes_refusals(fe_pkg):
    pkg = fe_pkg
    L = pkg.fe_lib()

    def rc(fe, echoes, n=None):
        arr = (pkg.Echo * max(len(echoes), 1))(*[pkg.Echo(*e) for e in echoes])
        return L.gpsfe_set_echoes(fe._fe, arr, len(echoes) if n is None else n)

    fe = front_end(pkg)
    good = (5, 10.0, 3.0)
    assert rc(fe, [good]) == 0 and fe.block_chans == 13
    assert rc(fe, [good, good]) == 0 and fe.block_chans == 14       # two echoes of one PRN; a second call replaces the first
    for bad in ((0, 10.0, 3.0), (33, 10.0, 3.0), (-1, 10.0, 3.0), (5, -1.0, 3.0), (5, float("nan"), 3.0), (5, float("inf"), 3.0),
                (5, 30000.5, 3.0), (5, 10.0, float("nan")), (5, 10.0, 3.0, float("inf")), (5, 10.0, 3.0, 0.0, float("nan"))):
        assert rc(fe, [good, bad]) == -1, bad
    assert fe.block_chans == 14                                      # a refused call changes nothing
    assert rc(fe, [(5, 30000.0, 3.0)]) == 0
    assert rc(fe, [good] * 5) == -1 and rc(fe, [good] * 4) == 0      # 12 + n <= 16
    assert rc(fe, [good], n=-1) == -1 and L.gpsfe_set_echoes(fe._fe, None, 1) == -1 and L.gpsfe_set_echoes(None, None, 0) == -1
    assert rc(fe, []) == 0 and fe.block_chans == 12
    fe.next_block()
    assert rc(fe, [good]) == -1 and rc(fe, []) == -1                  # after the first block
    with pytest.raises(RuntimeError):
        fe.set_echoes([good])
    fe.close()
    fe = front_end(pkg, max_chan=8)
    assert rc(fe, [good] * 8) == 0 and fe.block_chans == 16 and rc(fe, [good] * 9) == -1
    fe.generate(1)
    assert rc(fe, [good]) == -1
    fe.close()
    assert L.gpsfe_block_chans(None) == 0


def test_gpsbb_sim_takes_echoes(fe_pkg, tmp_path):
    """gpsbb-sim -M: named by the usage text, parsed (the tool says how many descriptors a block has before it touches a GPU),
    bad specs refused before anything is opened.  No GPU is needed: whether the run that follows finds a device is not looked at."""
    pkg = fe_pkg
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    nav = os.path.join(GOLDEN, "synth3540.14n")
    base = [exe, "-e", nav, "-l", "%g,%g,%g" % SITE, "-s", "2600000", "-n", "4096", "-d", "0.1", "-o", str(tmp_path / "out.bin")]

    def run(*args):
        return subprocess.run(list(args), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120, text=True)

    r = run(exe)
    assert r.returncode == 1 and "-M prn,extra_m,atten_db[,phase_cyc[,rate_mps]]" in r.stderr
    prn = 0
    fe = front_end(pkg)
    prn = int(fe.next_block()["prn"][0])
    fe.close()
    r = run(*base, "-M", "%d,345.9,6" % prn, "-M", "%d,20,3,0.25,1.5" % prn)
    assert "echoes: 2, 14 descriptors per block" in r.stderr, r.stderr
    r = run(*base, "-N", "8", *["-M", "%d,20,3" % prn] * 8)
    assert "echoes: 8, 16 descriptors per block" in r.stderr, r.stderr
    for bad in (["-M", "0,10,3"], ["-M", "33,10,3"], ["-M", "5,10"], ["-M", "5,-1,3"], ["-M", "5,30001,3"], ["-M", "5,10,3,0,0,0"],
                ["-M", "5,10,x"], ["-M", "5.5,10,3"], ["-M", "5,10,3,"], ["-M", "5,nan,3"], ["-M", "1e30,10,3"], ["-M", "-1e30,10,3"], ["-M", "5,10,3"] * 5, ["-N", "8"] + ["-M", "5,10,3"] * 9):
        r = run(*base, *bad)
        assert r.returncode == 1 and "-M wants" in r.stderr, (bad, r.stderr)
        assert "echoes:" not in r.stderr
