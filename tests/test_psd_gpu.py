"""gpsbb_device_psd on the GPU (k_psd, k_psd_fold): every comparison is == on all N bins and the segment count against psd_host fed
with view_host's output (tools/psd_check.py), on the smallest shapes at which the kernel can go wrong — every transform length,
hops below, at and above it, segment counts around one and two workgroup runs, the range's end, every view and impairment, a call
split in two, every refusal, large and small calls interleaved with the other calls that read device IQ — and end to end: what a
CW emitter, a chirp, the front-end filter's stop band and the level look like in the bins."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import psd_check as pc  # noqa: E402
from psd_check import ac, fc, tc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1


def clips(pkg, synth):
    return synth.info(pkg.INFO_SC8_CLIPPED), synth.info(pkg.INFO_NOISE_CLIPPED)


@pytest.mark.parametrize("log2n", pc.LOG2NS)
def test_1_stage_and_lane_map(pkg, synth, log2n):
    """Random full-range int16 IQ with 32767, -32767 and -32768 in it under a random full-range window with -32768 in it; hops 1,
    N / 2, N and N + 3; segment counts 1, 2, 5, and one below, at and one above one and two workgroup runs."""
    N = 1 << log2n
    r = pkg.psd_run(log2n)
    assert r == pkg.exp_lib().gpsbb_test_psd_run(log2n) and {1, 2, 5, r, r + 1, 2 * r, 2 * r + 1} <= set(pc.counts(pkg, log2n))
    big = ac.random_iq(64, 0x9500 + log2n)
    assert {32767, -32767, -32768} <= set(big[:, 0].tolist()) and -32768 in pc.random_window(N, 0x9D00 + log2n).tolist()
    bad = pc.lane_map(pkg, synth, log2n)
    assert not bad, "\n".join(bad)


def test_2_ends(pkg, synth):
    """Spare samples of 0x7fff behind the buffer enter no sum; nsamp = N gives one segment, N + hop - 1 still one, N + hop two."""
    N, hop = 512, 300
    iq = ac.random_iq(N + hop, 0x9E1)
    iq7 = np.concatenate([iq, np.full((7, 2), 0x7FFF, np.int16)])
    p = pkg.Psd(9, hop, 0, pc.random_window(N, 0x9E2))
    bad = []
    for n, want_nseg in ((N, 1), (N + hop - 1, 1), (N + hop, 2)):
        got = pc.on_device(pkg, synth, iq7, p, nsamp=n)
        bad += pc.compare(got, pc.mirror(pkg, iq, p, nsamp=n), "nsamp %d" % n)
        assert got[1] == want_nseg
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("log2n", [6, 9, 12])
def test_3_range(pkg, synth, log2n):
    """Every component -32768 under a window of all -32768 in SC16: seven segments at shift 0 give psd[0] == 7 * 2 * 2^58 and every
    other bin 0, and == the mirror.  Eight segments at shift 0 are refused and are served at shift 1."""
    N = 1 << log2n
    iq = np.full((8 * N, 2), -32768, np.int16)
    p = pkg.Psd(log2n, N, 0, np.full(N, -32768, np.int16))
    got = pc.on_device(pkg, synth, iq, p, nsamp=7 * N)
    bad = pc.compare(got, pc.mirror(pkg, iq, p, nsamp=7 * N))
    assert not bad, "\n".join(bad)
    assert got[1] == 7 and int(got[0][0]) == 7 * 2 * (1 << 58) and not got[0][1:].any()
    with pytest.raises(pkg.GpsbbError) as e:
        pc.on_device(pkg, synth, iq, p)
    assert e.value.rc == BADARG
    p1 = p.copy(shift=1)
    got = pc.on_device(pkg, synth, iq, p1)
    assert not pc.compare(got, pc.mirror(pkg, iq, p1))
    assert got[1] == 8 and int(got[0][0]) == 8 * 2 * (1 << 56) and not got[0][1:].any()


@pytest.mark.parametrize("impair", ["plain", "noise", "noise+chirp", "chirp"])
@pytest.mark.parametrize("view", ["sc16", "sc8", "sc1"])
def test_4_views(pkg, synth, view, impair):
    """SC16, SC8(3) and SC1, each plain, with a gpsbb_noise_t whose sample0 lies above 2^32, with noise and a chirp, with the chirp
    alone.  The handle's clip counters do not move; the impaired spectrum differs from the plain one."""
    fmt = {"sc16": pkg.OUT_SC16, "sc8": pkg.OUT_SC8(3), "sc1": pkg.OUT_SC1}[view]
    iq = (ac.random_iq(256 + 40 * 128, 0x9C1).astype(np.int32) // 4).astype(np.int16)   # (room for the impairments)
    p = pkg.psd_make(8, iq.shape[0], 0, pkg.PSD_HANN)
    nz = pkg._as_noise(pc.NOISE) if "noise" in impair else None
    js = pc.chirp_set(pkg) if "chirp" in impair else None
    assert pc.NOISE["sample0"] > 1 << 32
    before = clips(pkg, synth)
    got = pc.on_device(pkg, synth, iq, p, fmt, nz, js)
    bad = pc.compare(got, pc.mirror(pkg, iq, p, fmt, nz, js), "%s %s" % (view, impair))
    assert not bad, "\n".join(bad)
    assert clips(pkg, synth) == before and got[1] == 41
    if impair != "plain":
        assert (got[0] != pc.mirror(pkg, iq, p, fmt)[0]).any()


def test_5_split(pkg, synth):
    """With noise on: one call == the bin-wise sum of two calls split at segment k, sample k * hop, sample0 advanced by as much: a
    k inside a workgroup's run and one at a run's boundary."""
    log2n, N, hop = 8, 256, 128
    r = pkg.psd_run(log2n)
    nseg = 3 * r + 3
    iq = (ac.random_iq(pc.nsamp_for(N, hop, nseg), 0x9B1).astype(np.int32) // 4).astype(np.int16)
    p = pkg.Psd(log2n, hop, pkg.psd_min_shift(nseg), pc.random_window(N, 0x9B2))
    whole = pc.on_device(pkg, synth, iq, p, noise=pc.NOISE)
    bad = pc.compare(whole, pc.mirror(pkg, iq, p, noise=pc.NOISE), "whole")
    assert whole[1] == nseg
    for k in (3, r):
        nz, _ = pc.advanced(pkg, pc.NOISE, None, k * hop)
        a = pc.on_device(pkg, synth, iq[:pc.nsamp_for(N, hop, k)], p, noise=pc.NOISE)
        b = pc.on_device(pkg, synth, iq[k * hop:], p, noise=nz)
        assert (a[1], b[1]) == (k, nseg - k)
        bad += pc.compare((a[0] + b[0], a[1] + b[1]), whole, "split at %d" % k)
    assert not bad, "\n".join(bad)


def test_6_refusals(pkg, synth, oracle):
    """Every GPSBB_E_BADARG of the definition and the served neighbour of each; after every refusal psd and nseg_out are as they
    were and the handle still renders a block bit-exactly."""
    import torch
    L = pkg.lib()
    n = 4096 + 64
    t = torch.zeros((n + 8, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    good = pkg.psd_make(6, n)
    ch = pkg.synth_descriptors(1, nch=4, seed=31)[0]
    delt = 1.0 / pc.FS
    want_iq = oracle.fill_blocks(ch[None, :], delt, 1500)[0][0]
    out = np.full(4096, 0x77, np.uint64)
    nseg = C.c_long(12345)

    def rc(p=good, src=t.data_ptr(), nsamp=n, view=0, nz=None, js=None, null_p=False, null_out=False, h=None):
        r = L.gpsbb_device_psd(synth._h if h is None else h, C.c_void_p(src) if src else None, nsamp, view, None if nz is None else C.byref(nz),
                               None if js is None else C.byref(js), None if null_p else C.byref(p), None if null_out else out.ctypes.data,
                               C.byref(nseg))
        if r != 0:
            assert (out == 0x77).all() and nseg.value == 12345
        return r

    def still_renders():
        iq, _ = synth.fill_block(ch, delt, 1500)
        assert (iq == want_iq).all()

    def served(want_nseg=None, **kw):
        r = rc(**kw)
        ok = r == 0 and nseg.value != 12345 and (want_nseg is None or nseg.value == want_nseg)
        out[:] = 0x77
        nseg.value = 12345
        return ok

    assert served()
    still_renders()
    nz_ok = pkg.Noise(1, 5, 100.0, 1, 0)
    cw = pkg.interf_make(pkg.INTERF_CW, 0.0, 1000.0, delt=delt)
    js5 = pkg.InterfSet([cw], 0, 0)
    js5.n = 5
    cases = [("d_iq NULL", dict(src=0)), ("p NULL", dict(null_p=True)), ("psd NULL", dict(null_out=True)), ("d_iq misaligned", dict(src=t.data_ptr() + 2)),
             ("nsamp < N", dict(nsamp=63)), ("nsamp 0", dict(nsamp=0)), ("nsamp < 0", dict(nsamp=-64)),
             ("log2n 5", dict(p=good.copy(log2n=5))), ("log2n 13", dict(p=good.copy(log2n=13))), ("hop 0", dict(p=good.copy(hop=0))),
             ("hop -1", dict(p=good.copy(hop=-1))), ("hop beyond", dict(p=good.copy(hop=(1 << 20) + 1))), ("shift -1", dict(p=good.copy(shift=-1))),
             ("shift 31", dict(p=good.copy(shift=31))), ("eight segments at shift 0", dict(p=good.copy(shift=0), nsamp=8 * 64)),
             ("the plan's segments one shift below", dict(p=good.copy(shift=good.shift - 1))),
             ("a view with a flag", dict(view=pkg.OUT_SC16 | 1)), ("format 3", dict(view=0x300)), ("a shift on SC16", dict(view=0x3000)),
             ("noise sigma 0", dict(nz=pkg.Noise(1, 0, 0.0, 0, 0))), ("noise shift 8", dict(nz=pkg.Noise(1, 0, 100.0, 8, 0))),
             ("a set of 5 emitters", dict(js=js5)), ("a set's shift 8", dict(js=pkg.InterfSet([cw], 8, 0))),
             ("noise and set apart in sample0", dict(nz=nz_ok, js=pkg.InterfSet([cw], 1, 6))),
             ("noise and set apart in shift", dict(nz=nz_ok, js=pkg.InterfSet([cw], 2, 5)))]
    assert good.shift >= 1
    for what, kw in cases:
        assert rc(**kw) == BADARG, what
        still_renders()
    assert rc(h=0) == BADARG
    # more than 2^20 segments: a buffer of its own, hop 1
    big = torch.zeros((64 + (1 << 20) + 8, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    dense = good.copy(hop=1, shift=30)
    assert rc(p=dense, src=big.data_ptr(), nsamp=64 + (1 << 20)) == BADARG
    still_renders()
    assert served(1 << 20, p=dense, src=big.data_ptr(), nsamp=64 + (1 << 20) - 1)
    # the neighbours of the refusals are served
    assert served(1, nsamp=64) and served(p=good.copy(log2n=12, hop=4096, shift=0), want_nseg=1) and served(1, p=good.copy(hop=1 << 20))
    assert served(p=good.copy(hop=1, shift=30), want_nseg=n - 63) and served(p=good.copy(shift=30)) and served(7, p=good.copy(shift=0), nsamp=7 * 64)
    assert served(8, p=good.copy(shift=1), nsamp=8 * 64) and served(view=pkg.OUT_SC8(7)) and served(view=pkg.OUT_SC1)
    assert served(nz=nz_ok, js=pkg.InterfSet([cw], 1, 5)) and served(nz=nz_ok) and served(js=pkg.InterfSet([cw], 1, 5))
    assert L.gpsbb_device_psd(synth._h, C.c_void_p(t.data_ptr()), n, 0, None, None, C.byref(good), out.ctypes.data, None) == 0   # nseg_out NULL
    still_renders()


def test_7_interleaved(pkg, synth):
    """Large, small, large on one handle with a device_fir and a device_acquire call between them: the scratch is kept between
    calls, every spectrum == the mirror and the neighbours' results == theirs."""
    import torch
    big_iq = ac.random_iq(pc.nsamp_for(4096, 1024, 37), 0x971)
    big = pkg.Psd(12, 1024, pkg.psd_min_shift(37), pc.random_window(4096, 0x972))
    small_iq = ac.random_iq(64, 0x973)
    small = pkg.Psd(6, 64, 0, pc.random_window(64, 0x974))
    want_big, want_small = pc.mirror(pkg, big_iq, big), pc.mirror(pkg, small_iq, small)
    fir_iq, fir = ac.random_iq(4096, 0xF129), fc.random_fir(pkg, 129, 16, 12, 0xF16)
    acq_iq, acq = ac.lane_map_case(pkg)
    want_fir, want_acq = fc.mirror(pkg, fir_iq, fir), pkg.acquire_host(pkg.view_host(acq_iq), acq)
    bad = pc.compare(pc.on_device(pkg, synth, big_iq, big), want_big, "large")
    bad += fc.compare(fc.on_device(pkg, synth, fir_iq, fir), want_fir, "fir")
    bad += pc.compare(pc.on_device(pkg, synth, small_iq, small), want_small, "small")
    t = torch.from_numpy(acq_iq).cuda()
    torch.cuda.synchronize()
    bad += ac.compare(synth.device_acquire(t.data_ptr(), acq_iq.shape[0], acq), None, want_acq[0], None, "acquire")
    bad += pc.compare(pc.on_device(pkg, synth, big_iq, big), want_big, "large again")
    assert not bad, "\n".join(bad)


def rendered(pkg, synth, ch, fs, nsamp):
    """(the batch, its device pointer, the render read back)"""
    b = synth.batch(ch, 1.0 / fs, nsamp)
    b.run()
    synth.sync()
    iq, _ = b.read()
    return b, b.device_iq(), iq[0]


def test_8a_cw_on_a_bin(pkg, synth):
    """Six satellites (tools/track_check.e2e_descriptors) at 2.6 MS/s and one CW emitter 20 dB above a gain-1.0 channel on the centre
    of bin +100 (253.9 kHz), then of bin -100: under Hann at N = 1024 the largest bin is 100, respectively 924; == the mirror."""
    ch = pc.e2e_descriptors(pkg)
    b, d_iq, iq = rendered(pkg, synth, ch, pc.FS, pc.E2E_NSAMP)
    try:
        p = pc.hann_plan(pkg, pc.E2E_NSAMP)
        for k0 in (pc.E2E_K0, -pc.E2E_K0):
            js = pc.cw_set(pkg, k0)
            got = synth.device_psd(d_iq, pc.E2E_NSAMP, p, interf=js)
            bad = pc.compare(got, pc.mirror(pkg, iq, p, interf=js), "CW at bin %d" % k0)
            assert not bad, "\n".join(bad)
            print("CW at bin %d: largest bin %d, %d segments" % (k0, int(np.argmax(got[0])), got[1]))
            assert int(np.argmax(got[0])) == k0 % pc.E2E_N and got[1] == 32
    finally:
        b.close()


def test_8b_chirp_fills_its_band(pkg, synth):
    """The same render with a chirp over [300, 700] kHz at J/S 10 dB: the share of sum(psd) in the band's bins, less the same share
    without the emitter, is positive and at least half of P_J / (P_J + P_S), P_J = 10^(J/S / 10) and P_S the sum of the channels'
    squared gains (an emitter of level g has the power of a channel of gain g).  On the mirror: 0.866 - 0.176 against 0.853."""
    ch = pc.e2e_descriptors(pkg)
    b, d_iq, iq = rendered(pkg, synth, ch, pc.FS, pc.E2E_NSAMP)
    try:
        p = pc.hann_plan(pkg, pc.E2E_NSAMP)
        js = pc.band_set(pkg)
        plain, band = synth.device_psd(d_iq, pc.E2E_NSAMP, p), synth.device_psd(d_iq, pc.E2E_NSAMP, p, interf=js)
        bad = pc.compare(plain, pc.mirror(pkg, iq, p), "plain") + pc.compare(band, pc.mirror(pkg, iq, p, interf=js), "chirp")
        assert not bad, "\n".join(bad)
        gain, want = pc.band_share(band[0]) - pc.band_share(plain[0]), pc.predicted_share(pkg, ch, pc.E2E_CHIRP[2])
        print("share in band %.4f, without %.4f, predicted %.4f" % (pc.band_share(band[0]), pc.band_share(plain[0]), want))
        assert gain > 0 and gain >= 0.5 * want
    finally:
        b.close()


def test_8c_stop_band_through_the_filter(pkg, synth):
    """A zeroed buffer at 10.4 MS/s given one CW emitter (amplitude 27 000: below the view's clamp) by device_impair on the centre
    of bin 153 of N = 1024, 1553.9 kHz, where fir_check.response_db of fir_check.e2e_fir says -40.78 dB; the spectrum there before
    the filter, and at bin 612, where the tone aliases to, after device_fir to 2.6 MS/s: the drop in dB equals the response within
    0.25 dB.  Both spectra == the mirror's, and on the mirror the drop is 40.774 dB, 0.008 dB from the response: the filter's
    output rounding (an amplitude of 250 after it) and the emitter's 9-bit phase, no leakage on a bin centre."""
    import torch
    fir = fc.e2e_fir(pkg)
    k, db, kout = pc.stop_band_bin(pkg, fir)
    assert abs(db + 40.0) < 1.0 and pc.E2E_MARGIN_DB <= 1.0
    n_in = pc.E2E_FIR_NSAMP_IN
    js = pc.cw_set(pkg, k, pc.E2E_TONE_JS_DB, fc.FS_IN)
    src = torch.zeros((n_in, 2), dtype=torch.int16, device="cuda")
    dst = torch.zeros((n_in // 4, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    synth.device_impair(src.data_ptr(), 1, n_in, None, js)
    pin, pout = pc.hann_plan(pkg, n_in), pc.hann_plan(pkg, n_in // 4)
    a = synth.device_psd(src.data_ptr(), n_in, pin)
    _, clipped = synth.device_fir(src.data_ptr(), n_in, fir, dst.data_ptr())
    bq = synth.device_psd(dst.data_ptr(), n_in // 4, pout)
    w, y = src.cpu().numpy(), dst.cpu().numpy()
    bad = pc.compare(a, pc.mirror(pkg, w, pin), "before") + pc.compare(bq, pc.mirror(pkg, y, pout), "after")
    assert not bad, "\n".join(bad)
    assert (w == pkg.view_host(np.zeros((n_in, 2), np.int16), interf=js)).all() and (y == pkg.fir_host(w, fir)[0]).all() and clipped == 0
    drop = pc.bin_db(a[0], pin, a[1], k) - pc.bin_db(bq[0], pout, bq[1], kout)
    print("bin %d -> %d: response %.3f dB, drop %.3f dB" % (k, kout, db, drop))
    assert int(np.argmax(a[0])) == k   # (after the filter the tone is 40 dB down and no longer the largest bin: bin 0 passes unchanged)
    assert abs(drop + db) <= pc.E2E_MARGIN_DB


def test_8d_sum_of_bins_is_the_level(pkg, synth):
    """sum(psd) * psd_scale under the rectangular window against the exact sum of squares gpsbb_device_level reports for the same
    samples, within the 1e-4 of the CPU test (on the mirror: 2.5e-8)."""
    ch = pc.e2e_descriptors(pkg)
    b, d_iq, iq = rendered(pkg, synth, ch, pc.FS, pc.E2E_NSAMP)
    try:
        n = pc.E2E_NSAMP // pc.E2E_N * pc.E2E_N
        p = pkg.psd_make(pc.E2E_LOG2N, n)
        got = synth.device_psd(d_iq, n, p)
        bad = pc.compare(got, pc.mirror(pkg, iq, p, nsamp=n))
        assert not bad, "\n".join(bad)
        lv = synth.device_level(d_iq, 1, n)
        exact = float(int(lv["sumsq"][0, 0]) + int(lv["sumsq"][0, 1])) / n
        est = float(got[0].astype(np.float64).sum()) * pkg.psd_scale(p, got[1])
        print("sum of the bins %.6g, the level's mean square %.6g: %.2e" % (est, exact, est / exact - 1))
        assert int(lv["n"][0]) == n and got[1] == n // pc.E2E_N and abs(est / exact - 1) <= 1e-4
    finally:
        b.close()
