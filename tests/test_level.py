"""The output level on the CPU (include/gpsbb.h gpsbb_level_t): level_host against Python integers, the layout, the two clip
identities of gpsbb_level_clips against apply_impair and SC8's clamp for every (shift, shift8), gpsbb_level_choose against a
numpy restatement, and the scenario of tests/test_despread.py end to end: what the chosen shifts cost in C/N0, and what the
command line's default costs under a jammer."""
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_check as dc  # noqa: E402


def boundary_values(kmax):
    """0, -1, +-1, and +-2^k, 2^k - 1, -2^k - 1 for k up to kmax"""
    v = [0, -1, 1]
    for k in range(kmax + 1):
        v += [1 << k, -(1 << k), (1 << k) - 1, -(1 << k) - 1]
    return v


def bitlen(x):
    return x.bit_length() if x >= 0 else (~x).bit_length()


def test_level_host_against_python_integers(pkg):
    rng = np.random.default_rng(21)
    v = boundary_values(23)
    v += [int(t) for t in rng.integers(-(1 << 24), (1 << 24) + 1, 2000 - len(v))]
    assert len(v) == 2000
    x = np.array(v, np.int64).reshape(1, 1000, 2)
    got = pkg.level_host(x)
    assert got.dtype == pkg.LEVEL_DTYPE and got.shape == (1,) and int(got["n"][0]) == 1000
    for c in range(2):
        want = [0] * pkg.LEVEL_CLASSES
        sq = 0
        for t in v[c::2]:
            want[bitlen(t)] += 1
            sq += t * t
        assert [int(t) for t in got["hist"][0, c]] == want
        assert int(got["sumsq"][0, c]) == sq
    assert bitlen(0) == bitlen(-1) == 0 and bitlen(32767) == bitlen(-32768) == 15 and bitlen(-(1 << 23) - 1) == 24
    # two blocks, int16: per block
    iq = rng.integers(-32768, 32768, (2, 77, 2)).astype(np.int16)
    two = pkg.level_host(iq)
    for b in range(2):
        assert (two[b:b + 1].tobytes() == pkg.level_host(iq[b]).tobytes())
        assert int(two["hist"][b].sum()) == 2 * 77


def test_layout(pkg):
    assert C.sizeof(pkg.Level) == 536 and pkg.LEVEL_DTYPE.itemsize == 536
    for name in ("n", "sumsq", "hist"):
        assert pkg.LEVEL_DTYPE.fields[name][1] == getattr(pkg.Level, name).offset


def clips_numpy(lv, a, shift8):
    """the header's identities on the histogram"""
    h = lv["hist"].astype(np.int64).sum(axis=(0, 1))
    m = np.arange(h.shape[0])
    sat = int(h[m > 15 + a].sum())
    c8 = int(h[(m - a > 7 + shift8) & (m <= 15 + a)].sum()) + (sat if shift8 < 8 else 0)
    return sat, c8


def choose_numpy(lv, sc8, ppm):
    budget = math.floor(ppm * 1e-6 * float(2 * int(lv["n"].sum())))
    over = 0
    a = next((t for t in range(8) if clips_numpy(lv, t, 0)[0] <= budget), None)
    if a is None:
        a, over = 7, 1
    q = 0
    if sc8 and over:
        q = 15   # no shift meets the budget: both largest values
    elif sc8:
        q = next((t for t in range(16) if clips_numpy(lv, a, t)[1] <= budget), None)
        if q is None:
            q, over = 15, 1
    return a, q, over


def test_level_clips_for_every_pair(pkg, oracle):
    """one oracle block at 25 MS/s, noise at 45 dB-Hz plus a chirp at J/S 40: classes up to 17.  For all 8 x 16 pairs the two
    numbers are apply_impair's count and the count of w >> shift8 outside -128 .. 127."""
    fs, nsamp = 25e6, 20001
    delt = 1.0 / fs
    ch = pkg.synth_descriptors(1, nch=16, seed=71)
    iq, _, _ = oracle.fill_blocks(ch, delt, nsamp)
    sigma = pkg.noise_sigma(45.0, 1.0, delt)
    em = pkg.interf_make(pkg.INTERF_CHIRP, 40.0, -fs / 2, fs / 2, 1024 * delt, delt=delt)
    s0 = 999
    lv = pkg.level_host(iq, pkg.Noise(5, s0, sigma, 0, 0), pkg.InterfSet([em], 0, s0))
    top = max(k for k in range(pkg.LEVEL_CLASSES) if lv["hist"][0, :, k].any())
    assert top == 17, top
    for a in range(8):
        w, n16 = pkg.apply_impair(iq, pkg.Noise(5, s0, sigma, a, 0), pkg.InterfSet([em], a, s0))
        for q in range(16):
            s = w.astype(np.int32) >> q
            n8 = int(((s < -128) | (s > 127)).sum())
            assert pkg.level_clips(lv, a, pkg.OUT_SC8(q)) == (n16, n8), (a, q)
            assert clips_numpy(lv, a, q) == (n16, n8), (a, q)
            if (a, q) == (0, 0):
                assert n16 > 0 and n8 > 0
        assert pkg.level_clips(lv, a, pkg.OUT_SC16) == (n16, 0) and pkg.level_clips(lv, a, pkg.OUT_SC1) == (n16, 0)
    L = pkg.lib()
    for bad in ((None, 1, 0, 0), (lv.ctypes.data, 0, 0, 0), (lv.ctypes.data, 1, 8, 0), (lv.ctypes.data, 1, -1, 0),
                (lv.ctypes.data, 1, 0, 3 << 8), (lv.ctypes.data, 1, 0, pkg.OUT_SC1 | (2 << 12))):
        assert L.gpsbb_level_clips(*bad, None, None) == -1, bad
    assert abs(pkg.level_rms(lv, 0) - math.sqrt(int(lv["sumsq"][0, 0]) / nsamp)) < 1e-9 * pkg.level_rms(lv, 0)
    assert math.isnan(pkg.level_rms(lv, 2))


def test_level_choose(pkg):
    """the choice meets the budget, one shift less does not; the C function is the numpy restatement at 0, 100 and 10 000 ppm"""
    rng = np.random.default_rng(22)
    zeros = np.zeros((2, 50000, 2), np.int16)
    cases = []
    for sigma, seed in ((40.0, 1), (700.0, 2), (3000.0, 3), (10100.0, 4), (150000.0, 5)):
        cases.append(pkg.level_host(rng.integers(-3000, 3001, zeros.shape).astype(np.int16), pkg.Noise(seed, seed * 1000 + 1, sigma, 0, 0)))
    cases.append(pkg.level_host(zeros))
    cases.append(pkg.level_host(np.full((1, 10, 2), -1, np.int16)))
    for lv in cases:
        for ppm in (0.0, 100.0, 10000.0):
            budget = math.floor(ppm * 1e-6 * float(2 * int(lv["n"].sum())))
            for fmt, sc8 in ((pkg.OUT_SC8(0), True), (pkg.OUT_SC8(9), True), (pkg.OUT_SC16, False), (pkg.OUT_SC1, False)):
                a, q, met = pkg.level_choose(lv, fmt, ppm)
                assert (a, q, 0 if met else 1) == choose_numpy(lv, sc8, ppm), (ppm, hex(fmt))
                if not sc8:
                    assert q == 0
                if met:
                    c16, c8 = pkg.level_clips(lv, a, pkg.OUT_SC8(q) if sc8 else fmt)
                    assert c16 <= budget and c8 <= budget
                    if a > 0:
                        assert pkg.level_clips(lv, a - 1, pkg.OUT_SC16)[0] > budget
                    if sc8 and q > 0:
                        assert pkg.level_clips(lv, a, pkg.OUT_SC8(q - 1))[1] > budget
    assert pkg.level_choose(cases[-2], pkg.OUT_SC8(0), 100.0) == (0, 0, True)   # silence
    assert pkg.level_choose(cases[-1], pkg.OUT_SC8(0), 0.0) == (0, 0, True)     # -1 has bit length 0
    # the top sigma: class 23 starts at 4 sigma, a two-sided tail of 63 ppm, 12.7 of these 200 000 components (none with a
    # probability of 3e-6); a budget of 1 ppm is floor(0.2) = 0 components, which shift 7 cannot meet: 7 and 15 come back.
    big = pkg.level_host(zeros, pkg.Noise(9, 0, float(1 << 20), 0, 0))
    assert pkg.level_choose(big, pkg.OUT_SC8(0), 1.0) == (7, 15, False)
    assert pkg.level_clips(big, 7, pkg.OUT_SC8(15))[0] > 0
    L = pkg.lib()
    a, q = C.c_int(), C.c_int()
    for ppm in (float("nan"), -1.0):
        assert L.gpsbb_level_choose(big.ctypes.data, 2, pkg.OUT_SC16, ppm, C.byref(a), C.byref(q)) == -1
    assert L.gpsbb_level_choose(big.ctypes.data, 0, pkg.OUT_SC16, 100.0, C.byref(a), C.byref(q)) == -1
    assert L.gpsbb_level_choose(big.ctypes.data, 2, 3 << 8, 100.0, C.byref(a), C.byref(q)) == -1
    # only the format bits are read
    assert pkg.level_choose(cases[2], pkg.OUT_SC8(13) | 1, 100.0) == pkg.level_choose(cases[2], pkg.OUT_SC8(0), 100.0)


# ---- the scenario of tests/test_despread.py: what the choice is worth in C/N0 ---------------------------------------------
FS, NSAMP, NCH, NBLOCKS, SEG_TILES, CN0 = 2.6e6, 300000, 12, 10, 2, 45.0


def whole(p):
    w = p[:, :, :NSAMP // (1024 * SEG_TILES)]
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3).reshape(p.shape[1], -1, 2))


def test_the_chosen_shifts_lose_nothing(pkg, oracle):
    """2.6 MS/s, 12 channels of gain 0.3 - 0.8, one second, noise at 45 dB-Hz with seed 45; with and without a full-band chirp at
    J/S 30 dB.  The choice at 100 ppm is (0, 7) and (0, 8); the mean C/N0 found in the SC8 view at the chosen pair is within
    0.05 dB of the SC16 view's (seen: -0.005 and 0.000: the margin is ten times that, and a fifth of the smallest loss one
    shift below); with the jammer, OUT_SC8(5) — gpsbb-sim's default -q — loses more than 1 dB on every channel (seen: 5.2 - 6.3).
    The table of include/gpsbb.h's README row is printed."""
    delt = 1.0 / FS
    ch = pkg.synth_descriptors(NBLOCKS, nch=NCH, seed=45)
    ch["gain"] = ch["gain"][0]
    iq, _, _ = oracle.fill_blocks(ch, delt, NSAMP, chain=True)
    rep = dc.replicas(oracle, ch, delt, NSAMP, chain=True)
    nz = pkg.Noise(45, 0, pkg.noise_sigma(CN0, 1.0, delt), 0, 0)
    chirp = pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, 30.0, -FS / 2, FS / 2, 1024 * delt, delt=delt)], 0, 0)
    T = 1024 * SEG_TILES * delt

    def cn0(u):
        p = whole(pkg.despread_host(u, rep, SEG_TILES))
        return np.array([pkg.cn0_estimate(p[i], T) for i in range(NCH)])

    loss, chosen = {}, {}
    for col, js in (("noise only", None), ("chirp 30 dB", chirp)):
        lv = pkg.level_host(iq, nz, js)
        a, q, met = pkg.level_choose(lv, pkg.OUT_SC8(0), 100.0)
        assert met
        chosen[col] = (a, q)
        w = pkg.view_host(iq, pkg.OUT_SC16, nz, js)   # step 4 once per column; SC8's view of it is pack_iq's clamp (view_host's own)
        assert (pkg.view_host(iq[:1], pkg.OUT_SC8(5), nz, js) == pkg.pack_iq(w[:1].astype(np.int16), pkg.OUT_SC8(5))).all()
        ref = cn0(w)
        assert np.isfinite(ref).all()
        for sh in range(4, 11):
            loss[col, sh] = cn0(pkg.pack_iq(w.astype(np.int16), pkg.OUT_SC8(sh)).astype(np.int64)) - ref
    print("\nshift8   noise only   + chirp J/S 30 dB   (mean over %d channels of C/N0 in SC8 less C/N0 in SC16, dB)" % NCH)
    for sh in range(4, 11):
        print("%4d %12.3f%s %14.3f%s" % (sh, loss["noise only", sh].mean(), "*" if chosen["noise only"][1] == sh else " ",
                                          loss["chirp 30 dB", sh].mean(), "*" if chosen["chirp 30 dB"][1] == sh else " "))
    print("* chosen at 100 ppm: %r" % (chosen,))
    assert chosen == {"noise only": (0, 7), "chirp 30 dB": (0, 8)}
    for col in chosen:
        assert loss[col, chosen[col][1]].mean() > -0.05, (col, loss[col, chosen[col][1]])
    d5 = loss["chirp 30 dB", 5]
    print("OUT_SC8(5) under the chirp, per channel: %+.2f .. %+.2f dB" % (d5.min(), d5.max()))
    assert (d5 < -1.0).all(), d5
