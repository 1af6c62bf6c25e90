"""The tracking loops without a GPU: the numpy mirror's closing of an epoch (steps 4-8) against a term-by-term restatement in
Python integers, the host helpers (gpsbb_trk_make, gpsbb_trk_seed, gpsbb_trk_bitsync, gpsbb_trk_bits) against Python integers and
hand-made records, the mirror's own contract (resumable, the clamps reached), and end to end on the CPU oracle's render of six
satellites: acquired, tracked, their data bits read back."""
import ctypes as C
import math
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import track_check as tc  # noqa: E402

BADARG = -1
LEN = 1023 << 32
CMAX = (1 << 47) - 1


def tdiv(a, b):
    """the quotient rounded toward zero: the floor where it is positive, the ceiling where it is negative"""
    return a // b if (a < 0) == (b < 0) else -((-a) // b)


def bitlen(x):
    y, n = (x if x >= 0 else -x - 1), 0
    while y:
        y //= 2
        n += 1
    return n


def restated(cfg, st, cs, N, sums):
    """steps 4-8 once more, written from the header's text alone: -> (record fields, state fields after)"""
    m = max(bitlen(v) for v in sums)
    q = m - 20 if m > 20 else 0
    sh = [v // (1 << q) for v in sums]              # floor division: an arithmetic shift
    Ei, Eq, Pi, Pq, Li, Lq = sh
    E2 = Ei ** 2 + Eq ** 2
    L2 = Li ** 2 + Lq ** 2
    e_d = tdiv((E2 - L2) * 16384, E2 + L2 + 1)
    a = dict(st)
    if st["epoch"] < cfg.nfll:
        mode = 0
        if st["epoch"] == 0:
            e_c = 0
        else:
            cross = st["prev_i"] * Pq - st["prev_q"] * Pi
            dot = st["prev_i"] * Pi + st["prev_q"] * Pq
            e_c = tdiv((cross if dot >= 0 else -cross) * 16384, abs(dot) + abs(cross) + 1)
        a["carr_int"] = min(max(st["carr_int"] + cfg.kf * e_c, -CMAX), CMAX)
        a["carr_step"] = a["carr_int"]
    else:
        mode = 1
        e_c = tdiv((Pq if Pi >= 0 else -Pq) * 16384, abs(Pi) + abs(Pq) + 1)
        a["carr_int"] = min(max(st["carr_int"] + cfg.kp2 * e_c, -CMAX), CMAX)
        a["carr_step"] = min(max(a["carr_int"] + cfg.kp1 * e_c, -CMAX), CMAX)
    a["code_int"] = min(max(st["code_int"] + cfg.kd2 * e_d, -(1 << 56)), 1 << 56)
    a["code_adj"] = (a["code_int"] + cfg.kd1 * e_d) // 256
    s32 = (st["carr_step"] // 65536) % (1 << 32)
    a["carr_phase"] = (st["carr_phase"] + s32 * N) % (1 << 32)
    a["code_phase"] = st["code_phase"] + cs * N - LEN
    a["n0"] = st["n0"] + N
    a["epoch"] = st["epoch"] + 1
    a["prev_i"], a["prev_q"] = Pi, Pq
    rec = dict(n0=st["n0"], N=N, q=q, e_i=sums[0], e_q=sums[1], p_i=sums[2], p_q=sums[3], l_i=sums[4], l_q=sums[5],
               carr_step=st["carr_step"], code_phase=st["code_phase"], carr_phase=st["carr_phase"], e_c=e_c, e_d=e_d, mode=mode)
    return rec, a


def test_helpers_of_this_file():
    assert [tdiv(7, 2), tdiv(-7, 2), tdiv(7, -2), tdiv(-7, -2), tdiv(0, 5), tdiv(-1, 5)] == [3, -3, -3, 3, 0, 0]
    assert [bitlen(0), bitlen(-1), bitlen(1), bitlen(-2), bitlen((1 << 20) - 1), bitlen(1 << 20), bitlen(-(1 << 20)), bitlen(-(1 << 20) - 1)] == \
        [0, 0, 1, 1, 20, 21, 20, 21]


def test_1_closing_an_epoch_against_python_integers(pkg):
    """trk_close_host (what track_host runs per epoch) == the restatement above on random operands: negatives, zeros (0 / (0 + 1)),
    sums that make q > 0 and sums that do not, both modes, epoch 0, gains of either sign and at the ends of int32, states at the
    clamps."""
    rng = random.Random(0x7AC)
    big = (1 << 31) - 1
    seen_q, seen_q0, seen_zero, seen_clamp = 0, 0, 0, 0
    for it in range(3000):
        width = rng.choice((0, 3, 12, 20, 21, 30, 45))
        sums = [0 if width == 0 or rng.random() < 0.1 else rng.randint(-(1 << width), (1 << width) - 1) for _ in range(6)]
        if it % 7 == 0:
            sums[rng.randrange(6)] = rng.choice((-(1 << 20), (1 << 20) - 1, 1 << 20, -(1 << 20) - 1, -(1 << 45), (1 << 45)))
        gains = [rng.choice((0, 1, -1, big, -big - 1, rng.randint(-big, big), rng.randint(-100000, 100000))) for _ in range(5)]
        cfg = tc.make_cfg(pkg, code_nom=rng.randint(tc.smallest_code_nom(), 3 << 31), nfll=rng.choice((0, 1, 5)), gains=gains)
        lim = rng.choice((CMAX, 1 << 40, 1000))
        st = dict(prn=rng.randint(1, 32), epoch=rng.choice((0, 1, 4, 5, 6, 1000)), n0=rng.randint(0, 1 << 40), carr_phase=rng.getrandbits(32),
                  _pad=0, carr_int=rng.randint(-lim, lim), carr_step=rng.randint(-lim, lim), code_phase=rng.randrange(LEN),
                  code_int=rng.choice((0, 1 << 56, -(1 << 56), rng.randint(-(1 << 56), 1 << 56))), code_adj=rng.randint(-(1 << 49), 1 << 49),
                  prev_i=rng.randint(-(1 << 20), (1 << 20) - 1), prev_q=rng.randint(-(1 << 20), (1 << 20) - 1))
        cs, N = rng.randint(1 << 22, 27 << 28), rng.randint(1, 1 << 20)
        want_rec, want_st = restated(cfg, st, cs, N, sums)
        got_st = dict(st)
        got_rec = pkg.trk_close_host(cfg, got_st, cs, N, sums)
        assert got_rec == want_rec, (it, sums)
        assert got_st == want_st, (it, sums)
        assert abs(got_rec["e_c"]) <= 1 << 14 and abs(got_rec["e_d"]) <= 1 << 14
        seen_q += got_rec["q"] > 0
        seen_q0 += got_rec["q"] == 0
        seen_zero += not any(sums)
        seen_clamp += abs(got_st["carr_step"]) == CMAX or abs(got_st["code_int"]) == 1 << 56
    assert seen_q > 500 and seen_q0 > 500 and seen_zero > 50 and seen_clamp > 50


def test_1b_plan_against_python_integers(pkg):
    """steps 1 and 2: cs inside its clamp, N the smallest count that carries code_phase to LEN or beyond"""
    rng = random.Random(5)
    for _ in range(2000):
        cfg = tc.make_cfg(pkg, code_nom=rng.randint(tc.smallest_code_nom(), 3 << 31), aid_div=rng.choice((0, 1, -1, 1540 << 16, -(1540 << 16), 7)))
        st = dict(carr_step=rng.randint(-CMAX, CMAX), code_adj=rng.randint(-(1 << 49), 1 << 49) >> rng.choice((0, 20, 30)), code_phase=rng.randrange(LEN))
        cs, N = pkg.trk_plan_host(cfg, st)
        nom = cfg.code_nom
        raw = nom + (tdiv(st["carr_step"], cfg.aid_div) if cfg.aid_div else 0) + st["code_adj"]
        assert cs == min(max(raw, nom - nom // 8), nom + nom // 8)
        assert N >= 1 and st["code_phase"] + cs * N >= LEN > st["code_phase"] + cs * (N - 1)
        assert N <= 1 << 20


@pytest.mark.parametrize("fs", [2.6e6, 25e6])
def test_2_make_against_python_floats(pkg, fs):
    delt = 1.0 / fs
    cfg = pkg.trk_make(delt)
    nom = int(np.rint(math.ldexp(1.023e6 * delt, 32)))
    nper = float(LEN) / nom
    T = nper * delt
    wn = 15.0 / 0.53
    want = dict(code_nom=nom, aid_div=1540 << 16, spacing=1 << 31, nfll=100, max_epochs=1000,
                kf=int(np.rint(0.15 * 2.0 ** 34 / (2 * math.pi * nper))), kp2=int(np.rint(wn * wn * T * delt / (2 * math.pi) * 2.0 ** 34)),
                kp1=int(np.rint(1.414 * wn * T / (2 * math.pi * nper) * 2.0 ** 34)), kd1=int(np.rint(0.1 * 2.0 ** 24 / nper)), kd2=0)
    assert {k: getattr(cfg, k) for k in want} == want
    if fs == 2.6e6:   # what the formulas give at nper = 2600; the prototype of the definition ran with 157755 and 42086, 6e-5 away
        assert (cfg.kf, cfg.kp1, cfg.kp2, cfg.kd1) == (157746, 42085, 842, 645)
    named = pkg.trk_make(delt, 0.3, 30.0, 0.2, 7, 55)
    assert (named.nfll, named.max_epochs) == (7, 55) and named.kd1 == int(np.rint(0.2 * 2.0 ** 24 / nper))
    assert abs(named.kf - 2 * cfg.kf) <= 1 and abs(named.kp1 - 2 * cfg.kp1) <= 1 and abs(named.kp2 - 4 * cfg.kp2) <= 2


def test_2_make_and_seed_refusals(pkg):
    L = pkg.lib()
    cfg = pkg.TrkCfg()
    cfg.nfll = 77   # (left as it was by every refusal)
    for what, args in (("delt 0", (0.0, 0, 0, 0, 0, 0)), ("delt NaN", (math.nan, 0, 0, 0, 0, 0)), ("delt inf", (math.inf, 0, 0, 0, 0, 0)),
                       ("fll_gain NaN", (1 / 2.6e6, math.nan, 0, 0, 0, 0)), ("pll_bw inf", (1 / 2.6e6, 0, math.inf, 0, 0, 0)),
                       ("dll_gain NaN", (1 / 2.6e6, 0, 0, math.nan, 0, 0)), ("max_epochs 2^20 + 1", (1 / 2.6e6, 0, 0, 0, 0, (1 << 20) + 1)),
                       ("more than 1.5 chips per sample", (2e-6, 0, 0, 0, 0, 0)), ("a code period above 2^20 samples", (1e-10, 0, 0, 0, 0, 0)),
                       ("a gain beyond int32", (1 / 2.6e6, 1e9, 0, 0, 0, 0))):
        assert L.gpsbb_trk_make(C.byref(cfg), *[float(a) if k < 4 else int(a) for k, a in enumerate(args)]) == BADARG, what
        assert cfg.nfll == 77
    assert L.gpsbb_trk_make(None, 1 / 2.6e6, 0.0, 0.0, 0.0, 0, 0) == BADARG
    assert L.gpsbb_trk_make(C.byref(cfg), 1 / 2.6e6, 0.0, 0.0, 0.0, 0, 1 << 20) == 0 and cfg.max_epochs == 1 << 20
    acq = pkg.acq_make(1 / 2.6e6, -5000.0, 250.0, 41, 1e-3, 0, 2)
    st = pkg.trk_seed(acq, 17, 3, 1234)
    want = np.zeros(1, pkg.TRK_STATE_DTYPE)[0]
    want["prn"], want["n0"], want["carr_int"], want["carr_step"] = 17, 1234, int(acq.step[3]) << 16, int(acq.step[3]) << 16
    assert st.tobytes() == want.tobytes() and acq.step[3] < 0
    assert int(pkg.trk_seed(acq, 1, 40, 0)["carr_step"]) == int(acq.step[40]) << 16 > 0
    buf = np.zeros(1, pkg.TRK_STATE_DTYPE)
    for what, (p, a, prn, b, lag) in (("state NULL", (None, acq, 1, 0, 0)), ("cfg NULL", (buf.ctypes.data, None, 1, 0, 0)),
                                      ("prn 0", (buf.ctypes.data, acq, 0, 0, 0)), ("prn 33", (buf.ctypes.data, acq, 33, 0, 0)),
                                      ("bin -1", (buf.ctypes.data, acq, 1, -1, 0)), ("bin nbins", (buf.ctypes.data, acq, 1, 41, 0)),
                                      ("lag -1", (buf.ctypes.data, acq, 1, 0, -1))):
        assert L.gpsbb_trk_seed(p, None if a is None else C.byref(a), prn, b, lag) == BADARG, what


def records(pkg, p_i):
    r = np.zeros(len(p_i), pkg.TRK_EPOCH_DTYPE)
    r["p_i"] = p_i
    return r


def test_2_bitsync_and_bits_on_hand_made_records(pkg):
    L = pkg.lib()
    # bits of 20 records that turn at index 7 mod 20: + - - + over records 7..86, a ragged last group
    signs = [1] * 7 + [-1] * 20 + [-1] * 20 + [1] * 20 + [-1] * 13
    r = records(pkg, [s * (1000 + k) for k, s in enumerate(signs)])
    off, hist = pkg.trk_bitsync(r, 0)
    assert off == 7 and hist.tolist() == [0] * 7 + [3] + [0] * 12    # changes at 7, 47, 67
    off, hist = pkg.trk_bitsync(r, 7)                                  # k in (skip, n): the change AT record 7 is not counted
    assert off == 7 and hist[7] == 2
    off, hist = pkg.trk_bitsync(r, 6)
    assert hist[7] == 3
    assert pkg.trk_bits(r, 7).tolist() == [-1, -1, 1]                  # the 13 records left over make no bit
    assert pkg.trk_bits(r, 7, 2).tolist() == [-1, -1]
    assert pkg.trk_bits(r, 0).tolist() == [-1, -1, 1, -1]              # 7+, 13-: the sum decides; ... ; 7+ 13-
    assert pkg.trk_bits(r, 61).tolist() == [] and pkg.trk_bits(r, 60).tolist() == [-1] and pkg.trk_bits(r, 1000).tolist() == []
    # a tie of the histogram goes to the lowest index; p_i == 0 counts as positive; a sum of 0 is a +1 bit
    r = records(pkg, [1, -1, 0, -1] + [-1] * 18 + [1, -1] + [5] * 10 + [-5] * 10)
    off, hist = pkg.trk_bitsync(r, 0)
    assert hist.tolist() == [0, 1, 2, 2, 1] + [0] * 9 + [1] + [0] * 5 and off == 2    # changes at records 1, 2, 3, 22, 23, 24, 34
    assert pkg.trk_bits(r, 24).tolist() == [1]
    off, hist = pkg.trk_bitsync(records(pkg, [3] * 50), 0)
    assert off == 0 and not hist.any()
    off, hist = pkg.trk_bitsync(records(pkg, []), 0)
    assert off == 0 and not hist.any() and pkg.trk_bits(records(pkg, []), 0).size == 0
    # sums near the records' range do not overflow: 20 x (2^45)
    assert pkg.trk_bits(records(pkg, [1 << 45] * 20 + [-(1 << 45)] * 20), 0).tolist() == [1, -1]
    one = records(pkg, [1, 2])
    bits = np.zeros(4, np.int8)
    for what, args in (("epochs NULL", (None, 2, 0, None, None)), ("n < 0", (one.ctypes.data, -1, 0, None, None)), ("skip < 0", (one.ctypes.data, 2, -1, None, None))):
        assert L.gpsbb_trk_bitsync(*args) == BADARG, what
    assert L.gpsbb_trk_bitsync(one.ctypes.data, 2, 0, None, None) == 0   # both out pointers may be NULL
    for what, args in (("epochs NULL", (None, 2, 0, bits.ctypes.data, 4)), ("bits NULL", (one.ctypes.data, 2, 0, None, 4)),
                       ("n < 0", (one.ctypes.data, -1, 0, bits.ctypes.data, 4)), ("first < 0", (one.ctypes.data, 2, -1, bits.ctypes.data, 4)),
                       ("max < 0", (one.ctypes.data, 2, 0, bits.ctypes.data, -1))):
        assert L.gpsbb_trk_bits(*args) == BADARG, what


def test_mirror_is_resumable_and_reaches_the_clamps(pkg):
    """What the GPU tests lean on, settled on the CPU first: the mirror over a buffer == the mirror in calls of 13, 1 and 26
    records; the clamps case's records show carr_step at +(2^47 - 1) and -(2^47 - 1) and cs at both ends of its clamp."""
    iq, cfg, st = tc.resume_case(pkg)
    u = pkg.view_host(iq, 0, tc.NOISE)
    whole = pkg.track_host(u, cfg, st)
    assert [r.size for r in whole[1]] == [40, 40, 40] and whole[1][0].tobytes() == whole[1][1].tobytes()
    s, parts = st, [[], [], []]
    for n in (13, 1, 26):
        s, recs = pkg.track_host(u, cfg.copy(max_epochs=n), s)
        for c in range(3):
            assert recs[c].size == n
            parts[c].append(recs[c])
    assert not tc.compare((s, [np.concatenate(p) for p in parts]), whole)
    assert (whole[1][2]["mode"] == [0] * 20 + [1] * 20).all()
    iq, cfg, st = tc.clamps_case(pkg)
    s, recs = pkg.track_host(pkg.view_host(iq), cfg, st)
    steps = [int(v) for r in recs for v in r["carr_step"]] + [int(v) for v in s["carr_step"]]
    assert CMAX in steps and -CMAX in steps and [r.size for r in recs] == [10, 10]
    nom = cfg.code_nom
    cs = [v for c in range(2) for v in tc.records_cs(recs[c], s[c])]
    assert nom - nom // 8 in cs and nom + nom // 8 in cs


def test_mirror_stops_at_the_buffers_end(pkg):
    iq, cfg, st = tc.ends_case(pkg)
    s5, r5 = pkg.track_host(pkg.view_host(iq), cfg.copy(max_epochs=5), st)
    n_end = int(s5["n0"][0])
    s, r = pkg.track_host(pkg.view_host(iq[:n_end]), cfg, st)
    assert r[0].size == 5 and s[0].tobytes() == s5[0].tobytes()
    s, r = pkg.track_host(pkg.view_host(iq[:n_end - 1]), cfg, st)
    s4, _ = pkg.track_host(pkg.view_host(iq), cfg.copy(max_epochs=4), st)
    assert r[0].size == 4 and s[0].tobytes() == s4[0].tobytes()


@pytest.mark.parametrize("name", ["sc16", "sc1"])
def test_3_end_to_end_on_the_oracles_render(pkg, oracle, name):
    """synth_descriptors(1, nch=6, seed=0xACC) rendered by the CPU oracle at 2.6 MS/s in one block of 1 300 000 samples.
    acquire_host on its first 7800 samples (41 bins of 250 Hz, 2 x 1 ms; the mask cut to the six present PRNs: the mirror's
    cost) seeds six channels, track_host follows them with trk_make's constants, and with skip = 150 per PRN: the mean carrier
    step of the last 50 epochs within 1 Hz of f_carr; one non-zero histogram bin, at (-(icode + 1)) mod 20; the 16 or 17 bits all
    equal or all opposite to dwrd's from (iword, ibit, icode), epoch 0 being code period icode + 1.  Prints min |P.i| and
    max |P.q| after epoch 150."""
    view = {"sc16": pkg.OUT_SC16, "sc1": pkg.OUT_SC1}[name]
    ch = tc.e2e_descriptors(pkg)
    iq = oracle.fill_blocks(ch, 1.0 / tc.FS, tc.E2E_NSAMP, chain=True)[0][0]
    acq = tc.e2e_acq_cfg(pkg, view)
    assert (acq.ncoh, acq.nlags, acq.nnc, acq.nbins) == (2600, 2600, 2, 41)
    u = pkg.view_host(iq, view)
    rows, _ = pkg.acquire_host(u[:tc.E2E_ACQ_NSAMP], acq.copy(prn_mask=tc.ac.mask_of(tc.E2E_PRESENT)))
    st = tc.e2e_seeds(pkg, rows, acq)
    _, recs = pkg.track_host(u, tc.e2e_trk_cfg(pkg), st)
    bad, (min_pi, max_pq) = tc.e2e_findings(pkg, ch, recs)
    print("%s: min |P.i| %.3g, max |P.q| %.3g after epoch %d; records %s" % (name, min_pi, max_pq, tc.E2E_SKIP, [r.size for r in recs]))
    assert not bad, "\n".join(bad)
