"""The output level on the GPU (include/gpsbb.h gpsbb_level_t, k_level): gpsbb_device_level, GPSBB_PUSH_LEVEL and gpsbb-sim -A.
Every comparison is == against level_host (the numpy restatement) of the oracle's render or of a crafted buffer; the clip counts
predicted from one measurement are the growth of the library's own two counters."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BADARG, STATE = -1, -7
FS = 25e6
DELT = 1.0 / FS
S0 = (1 << 33) + 12345   # odd, above 2^32


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def emitters(pkg, delt):
    """tests/test_interf_gpu.py's four, restated: a tone; a full-band chirp of 1024 samples; a pulsed chirp whose sweep (301) and
    gate (260 / 78, offset 17) divide nothing; a pulsed tone at -fs/2 with a gate of 77"""
    fs = 1.0 / delt
    e1 = pkg.interf_make(pkg.INTERF_CW, -6.0, 1000.0, delt=delt)
    e1.phase0 = 0xFEDCBA9876543210
    e2 = pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -fs / 2, fs / 2, 1024 * delt, delt=delt)
    e3 = pkg.interf_make(pkg.INTERF_CHIRP, 0.0, -0.2 * fs, 0.27 * fs, 301 * delt, 260 * delt, 0.3, delt=delt)
    e3.pulse_offset, e3.phase0 = 17, 12345678901234567
    e4 = pkg.interf_make(pkg.INTERF_CW, 10.0, -fs / 2, pulse_period_s=77 * delt, duty=0.5, delt=delt)
    assert (e2.sweep, e3.sweep, e3.pulse_period, e3.pulse_on, e4.pulse_period) == (1024, 301, 260, 78, 77)
    return [e1, e2, e3, e4]


@pytest.fixture(scope="module")
def render(pkg, oracle):
    """16 channels at 25 MS/s, 3 x 20 001: the oracle's render, shared and left unchanged"""
    ch = pkg.synth_descriptors(3, nch=16, seed=0x1E7E1)
    iq, _, _ = oracle.fill_blocks(ch, DELT, 20001)
    iq.setflags(write=False)
    return iq


def crafted(nblocks, nsamp, seed):
    """every boundary value that fits int16 (0, -1, +-1, +-2^k, 2^k - 1, -2^k - 1), then a random fill"""
    rng = np.random.default_rng(seed)
    v = [0, -1, 1, 32767, -32768]
    for k in range(16):
        v += [t for t in (1 << k, -(1 << k), (1 << k) - 1, -(1 << k) - 1) if -32768 <= t <= 32767]
    a = rng.integers(-32768, 32768, nblocks * nsamp * 2).astype(np.int16)
    n = min(len(v), a.size)
    a[:n] = v[:n]
    a[a.size - n:] = v[:n][::-1]   # ... at the far end too: the last block's tail
    return a.reshape(nblocks, nsamp, 2)


# ---- plain --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nblocks,nsamp", [(3, 4099), (7, 1), (7, 3), (5, 5), (3, 20001)])
def test_plain_crafted(pkg, synth, nblocks, nsamp):
    """3 x 4 099: the blocks start at 0, 12 and 8 mod 16; nsamp 1, 3, 5: below one unit; 3 x 20 001: three chunks per block.
    Each also from a base 4 bytes off a 16-byte boundary."""
    iq = crafted(nblocks, nsamp, 31 + nsamp)
    want = pkg.level_host(iq)
    assert (want["n"] == nsamp).all() and int(want["hist"].sum()) == iq.size
    d = on_device(iq)
    assert d.data_ptr() % 16 == 0
    if nsamp == 4099:
        assert [(b * nsamp * 4) % 16 for b in range(3)] == [0, 12, 8]
    assert same(synth.device_level(d.data_ptr(), nblocks, nsamp), want)
    pad = np.zeros(iq.size + 2, np.int16)
    pad[2:] = iq.ravel()
    d2 = on_device(pad)
    assert (d2.data_ptr() + 4) % 16 == 4
    assert same(synth.device_level(d2.data_ptr() + 4, nblocks, nsamp), want)


# ---- noise, set, both ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["noise", "set", "both"])
def test_noise_set_both(pkg, synth, render, which):
    nz = pkg.Noise(77, S0, pkg.noise_sigma(45.0, 1.0, DELT), 0, 0) if which != "set" else None
    js = pkg.InterfSet(emitters(pkg, DELT), 0, S0) if which != "noise" else None
    want = pkg.level_host(render, nz, js)
    d = on_device(render)
    got = synth.device_level(d.data_ptr(), 3, 20001, nz, js)
    assert same(got, want), which
    assert not same(want, pkg.level_host(render))
    # the shift fields are checked and otherwise not used
    if which == "both":
        nz3, js3 = pkg.Noise(77, S0, nz.sigma, 3, 0), pkg.InterfSet(emitters(pkg, DELT), 3, S0)
        assert same(synth.device_level(d.data_ptr(), 3, 20001, nz3, js3), want)
    # an empty set with noise measures the noise alone
    if which == "noise":
        assert same(synth.device_level(d.data_ptr(), 3, 20001, nz, pkg.InterfSet([], 0, S0)), want)


def test_batch_level(pkg, synth, render):
    """Batch.level measures the batch's own buffer: the render is the oracle's"""
    ch = pkg.synth_descriptors(3, nch=16, seed=0x1E7E1)
    b = synth.batch(ch, DELT, 20001)
    b.run()
    synth.sync()
    nz = pkg.Noise(3, 5, 2000.0, 0, 0)
    assert same(b.level(noise=nz), pkg.level_host(render, nz))
    b.close()


# ---- the prediction against the library's own counters ------------------------------------------------------------------

def test_prediction_is_the_counters_growth(pkg, synth, render):
    nblocks, nsamp = 3, 20001
    tone = pkg.interf_make(pkg.INTERF_CW, 20 * math.log10(72.0), 2.5e5, delt=DELT)
    sigma = pkg.noise_sigma(45.0, 1.0, DELT)
    d = on_device(render)
    dst = on_device(np.zeros_like(render))
    lv = synth.device_level(d.data_ptr(), nblocks, nsamp, pkg.Noise(9, S0, sigma, 0, 0), pkg.InterfSet([tone], 0, S0))
    assert same(lv, pkg.level_host(render, pkg.Noise(9, S0, sigma, 0, 0), pkg.InterfSet([tone], 0, S0)))
    for a in (0, 1, 3):
        n0 = synth.info(pkg.INFO_NOISE_CLIPPED)
        synth.device_impair(d.data_ptr(), nblocks, nsamp, pkg.Noise(9, S0, sigma, a, 0), pkg.InterfSet([tone], a, S0), d_dst=dst.data_ptr())
        grown16 = synth.info(pkg.INFO_NOISE_CLIPPED) - n0
        for q in (2, 5, 9):
            c0 = synth.info(pkg.INFO_SC8_CLIPPED)
            synth.device_pack(dst.data_ptr(), nblocks, nsamp, pkg.OUT_SC8(q))
            grown8 = synth.info(pkg.INFO_SC8_CLIPPED) - c0
            assert pkg.level_clips(lv, a, pkg.OUT_SC8(q)) == (grown16, grown8), (a, q)
            if (a, q) == (0, 2):
                assert grown16 > 0 and grown8 > 0
    # the measurement itself moved neither counter
    n0, c0 = synth.info(pkg.INFO_NOISE_CLIPPED), synth.info(pkg.INFO_SC8_CLIPPED)
    synth.device_level(d.data_ptr(), nblocks, nsamp, pkg.Noise(9, S0, sigma, 0, 0), pkg.InterfSet([tone], 0, S0))
    assert (synth.info(pkg.INFO_NOISE_CLIPPED), synth.info(pkg.INFO_SC8_CLIPPED)) == (n0, c0)


# ---- the bound ---------------------------------------------------------------------------------------------------------------

def test_the_bound(pkg, synth):
    """four CW emitters of level_q16 2^27 in phase, no noise: B = 32768 + 4 * 2^20; nsamp * B^2 < 2^64 up to 1 032 3xx samples.
    The largest block accepted has its sum of squares, just under 2^64, equal to numpy's; one more sample is refused."""
    em = []
    for _ in range(4):
        e = pkg.Interf()
        e.kind, e.level_q16 = pkg.INTERF_CW, 1 << 27
        em.append(e)
    js = pkg.InterfSet(em, 0, 0)
    B = 32768 + 4 * (((1 << 27) * 512 + (1 << 15)) >> 16)
    assert B == 4227072
    nmax = ((1 << 64) - 1) // (B * B)
    assert nmax * B * B < 1 << 64 <= (nmax + 1) * B * B and 1.03e6 < nmax < 1.04e6
    rng = np.random.default_rng(41)
    iq = rng.integers(-32768, 32768, (1, nmax + 1, 2)).astype(np.int16)
    iq[0, :, 0] = 32767   # I at the top: x = B - 1 at every sample (cos512[0] = 512)
    d = on_device(iq)
    got = synth.device_level(d.data_ptr(), 1, nmax, interf=js)
    want = pkg.level_host(iq[:, :nmax], None, js)
    assert int(want["sumsq"][0, 0]) == nmax * (B - 1) ** 2 and (1 << 64) - 3 * B * B < nmax * (B - 1) ** 2 < 1 << 64
    assert same(got, want)
    out = np.zeros(1, pkg.LEVEL_DTYPE)
    assert pkg.lib().gpsbb_device_level(synth._h, C.c_void_p(d.data_ptr()), 1, nmax + 1, None, C.byref(js), out.ctypes.data) == BADARG
    assert same(synth.device_level(d.data_ptr(), 1, nmax, interf=js), want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(pkg, synth):
    L = pkg.lib()
    nblocks, nsamp = 2, 1003
    iq = crafted(nblocks, nsamp, 51)
    d = on_device(iq)
    p = C.c_void_p(d.data_ptr())
    nz = pkg.Noise(1, 100, 500.0, 0, 0)
    js = pkg.InterfSet(emitters(pkg, DELT)[:1], 0, 100)
    want = pkg.level_host(iq, nz, js)
    out = np.zeros(nblocks, pkg.LEVEL_DTYPE)
    o = out.ctypes.data
    bad = [
        ("out NULL", (p, nblocks, nsamp, C.byref(nz), C.byref(js), None)),
        ("nblocks < 1", (p, 0, nsamp, C.byref(nz), C.byref(js), o)),
        ("nsamp < 1", (p, nblocks, 0, C.byref(nz), C.byref(js), o)),
        ("2-byte aligned", (C.c_void_p(d.data_ptr() + 2), nblocks, nsamp - 1, C.byref(nz), C.byref(js), o)),
        ("sample0 apart", (p, nblocks, nsamp, C.byref(pkg.Noise(1, 101, 500.0, 0, 0)), C.byref(js), o)),
        ("shift apart", (p, nblocks, nsamp, C.byref(pkg.Noise(1, 100, 500.0, 1, 0)), C.byref(js), o)),
        ("shift 8", (p, nblocks, nsamp, C.byref(pkg.Noise(1, 100, 500.0, 8, 0)), None, o)),
        ("d_iq NULL", (None, nblocks, nsamp, None, None, o)),
    ]
    for name, args in bad:
        assert L.gpsbb_device_level(synth._h, *args) == BADARG, name
        assert not out.view(np.uint8).any(), name
        assert same(synth.device_level(d.data_ptr(), nblocks, nsamp, nz, js), want), name


# ---- the stream -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ring_render(pkg, oracle):
    """25 MS/s, nsamp 20 000, six chained blocks: three pushes of two"""
    ch = pkg.synth_descriptors(6, nch=16, seed=0x1E7E2)
    iq, _, _ = oracle.fill_blocks(ch, DELT, 20000, chain=True)
    iq.setflags(write=False)
    return ch, iq


@pytest.mark.parametrize("fmt_name", ["sc16", "sc8", "sc1"])
def test_stream_levels(pkg, synth, ring_render, fmt_name):
    ch, iq = ring_render
    fmt = {"sc16": pkg.OUT_SC16, "sc8": pkg.OUT_SC8(5), "sc1": pkg.OUT_SC1}[fmt_name]
    nsamp, bps = 20000, 2
    nz = pkg.Noise(13, S0, pkg.noise_sigma(45.0, 1.0, DELT), 1, 0)
    js = pkg.InterfSet(emitters(pkg, DELT), 1, S0)
    want = pkg.level_host(iq, nz, js)

    def run(level):
        s = synth.stream(16, DELT, nsamp, bps, depth=3, flags=pkg.CHAIN_CARRIER, fmt=fmt, noise=nz, interf=js)
        for k in range(3):
            s.push(ch[k * bps:(k + 1) * bps], level=level)
        out = [s.pop_level() if level else s.pop() for _ in range(3)]
        return s, out

    s0, plain = run(False)
    s0.close()
    s, flagged = run(True)
    for k in range(3):
        assert (flagged[k][0] == plain[k][0]).all(), k                              # the bytes of a push without the flag
        assert flagged[k][1].tobytes() == plain[k][1].tobytes()
        assert same(flagged[k][2], want[k * bps:(k + 1) * bps]), (fmt_name, k)      # positions carry on from push to push
    exp, _ = pkg.apply_impair(iq, nz, js)
    assert (np.concatenate([p[0] for p in plain]) == pkg.pack_iq(exp, fmt)).all()
    # after a reset they start again
    s.reset()
    s.push(ch[:bps], level=True)
    a, _, lv = s.pop_level()
    assert same(lv, want[:bps]) and (a == plain[0][0]).all()
    # pop_level on a push without the flag: GPSBB_E_STATE, the push still pending, and pop() takes it
    s.push(ch[bps:2 * bps])
    p = C.c_void_p()
    buf = np.zeros(bps, pkg.LEVEL_DTYPE)
    assert pkg.lib().gpsbb_stream_pop_level(s._s, C.byref(p), None, buf.ctypes.data) == STATE
    assert s.pending == 1
    b, _ = s.pop()
    assert (b == plain[1][0]).all()
    # levels NULL: gpsbb_stream_pop
    s.push(ch[2 * bps:], level=True)
    assert pkg.lib().gpsbb_stream_pop_level(s._s, C.byref(p), None, None) == 0 and s.pending == 0
    # with GPSBB_PUSH_DIGEST: refused, nothing pushed, and the stream goes on
    s.reset()
    assert pkg.lib().gpsbb_stream_push_ex(s._s, ch[:bps].ctypes.data, pkg.PUSH_LEVEL | pkg.PUSH_DIGEST) == BADARG
    assert s.pending == 0
    s.push(ch[:bps], level=True)
    a, _, lv = s.pop_level()
    assert same(lv, want[:bps]) and (a == plain[0][0]).all()
    s.close()


def test_stream_level_refused_on_a_device_only_ring(pkg, synth, ring_render):
    ch, iq = ring_render
    s = synth.stream(16, DELT, 20000, 2, depth=3, flags=pkg.CHAIN_CARRIER | pkg.STREAM_DEVICE_ONLY)
    assert pkg.lib().gpsbb_stream_push_ex(s._s, ch[:2].ctypes.data, pkg.PUSH_LEVEL) == BADARG
    assert s.pending == 0
    s.push(ch[:2])
    ptr, _ = s.pop()
    assert (synth.device_read(ptr, (2, 20000, 2)) == iq[:2]).all()
    assert same(synth.device_level(ptr, 2, 20000), pkg.level_host(iq[:2]))
    s.close()


# ---- gpsbb-sim -A ---------------------------------------------------------------------------------------------------------------

def sim(pkg, out, *args, check=True):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    r = subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100", "-s", "2600000",
                        *args, "-o", out], check=check, stderr=subprocess.PIPE, text=True, timeout=600)
    return r


AGC_LINE = re.compile(r"^agc: shift (\d+), q (\d+), rms ([0-9.]+) ([0-9.]+), predicted clips (\d+) (\d+) of (\d+) components \((\d+) blocks\)$",
                      re.M)


def test_gpsbb_sim_agc(pkg, synth, tmp_path):
    pkg.build_frontend()
    nsamp, fs = 300000, 2.6e6
    delt = 1.0 / fs
    sweep = 1024 * delt
    jarg = "chirp,30,%r,%r,%r" % (-fs / 2, fs / 2, sweep)
    auto = str(tmp_path / "auto.bin")
    err = sim(pkg, auto, "-d", "1", "-b", "8", "-W", "45", "-J", jarg, "-A", "100").stderr
    m = AGC_LINE.search(err)
    assert m, err
    a, q, c16, c8, ncomp, k = int(m[1]), int(m[2]), int(m[5]), int(m[6]), int(m[7]), int(m[8])
    assert k == 10 and ncomp == 2 * 10 * nsamp
    # the same ten blocks through the veneer
    plain = str(tmp_path / "plain.bin")
    sim(pkg, plain, "-d", "1", "-b", "16")
    iq16 = np.fromfile(plain, np.int16).reshape(10, nsamp, 2)
    nz = pkg.Noise(1, 0, pkg.noise_sigma(45.0, 1.0, delt), 0, 0)
    js = pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, 30.0, -fs / 2, fs / 2, sweep, delt=delt)], 0, 0)
    d = on_device(iq16)
    lv = synth.device_level(d.data_ptr(), 10, nsamp, nz, js)
    assert pkg.level_choose(lv, pkg.OUT_SC8(0), 100.0) == (a, q, True)
    assert pkg.level_clips(lv, a, pkg.OUT_SC8(q)) == (c16, c8) and max(c16, c8) <= math.floor(100e-6 * ncomp)
    assert abs(float(m[3]) - pkg.level_rms(lv, 0)) <= 0.05 and abs(float(m[4]) - pkg.level_rms(lv, 1)) <= 0.05
    # the file is the one of the explicit options, on the ring as well
    explicit = str(tmp_path / "explicit.bin")
    sim(pkg, explicit, "-d", "1", "-b", "8", "-W", "45,%d" % a, "-j", str(a), "-q", str(q), "-J", jarg)
    want = np.fromfile(explicit, np.int8)
    assert want.size == 10 * nsamp * 2 and (np.fromfile(auto, np.int8) == want).all()
    exp, _ = pkg.apply_impair(iq16, pkg.Noise(1, 0, nz.sigma, a, 0), pkg.InterfSet(list(js.e)[:1], a, 0))
    assert (want.reshape(10, nsamp, 2) == pkg.pack_iq(exp, pkg.OUT_SC8(q))).all()
    fast = str(tmp_path / "fast.bin")
    assert AGC_LINE.search(sim(pkg, fast, "-d", "1", "-b", "8", "-W", "45", "-J", jarg, "-A", "100", "-F").stderr)[2] == m[2]
    assert (np.fromfile(fast, np.int8) == want).all()
    # -A chooses the shifts itself
    for extra in (["-q", "5"], ["-j", "0"]):
        assert sim(pkg, str(tmp_path / "no.bin"), "-d", "0.1", "-b", "8", "-W", "45", "-J", jarg, "-A", "100", *extra, check=False).returncode != 0
    assert sim(pkg, str(tmp_path / "no.bin"), "-d", "0.1", "-b", "8", "-W", "45,1", "-A", "100", check=False).returncode != 0
