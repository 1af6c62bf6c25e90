"""gpsbb_device_excise on the GPU (k_excise, k_exc_fold): every comparison is == on every output sample, the history handed on and
both counters against excise_host fed with view_host's output (tools/exc_check.py), on the smallest shapes at which the kernel can
go wrong — every transform length, block counts around one and two workgroup runs, with and without a history, the range's end
and the clamp, every impairment, a call split inside a run and at a run's boundary, every refusal, calls interleaved with the other
calls that read device IQ — and end to end: a search that a CW emitter or a chirp defeats finds every satellite after excision."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import exc_check as ec  # noqa: E402
import psd_check as pc  # noqa: E402
from exc_check import ac, fc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1


def clips(pkg, synth):
    return synth.info(pkg.INFO_SC8_CLIPPED), synth.info(pkg.INFO_NOISE_CLIPPED)


@pytest.mark.parametrize("log2n", ec.LOG2NS)
def test_1_stage_and_lane_map(pkg, synth, log2n):
    """Random full-range int16 IQ with 32767 and -32768 in it under a random legal window with 0 and 16384 in it, about 10 % of the
    bins masked, thr at the median cell power; block counts 1, 2, 5, and one below, at and one above one and two workgroup runs;
    hist NULL and random."""
    N = 1 << log2n
    r = pkg.exc_run(log2n)
    assert r == pkg.exp_lib().gpsbb_test_exc_run(log2n) and {1, 2, 5, r, r + 1, 2 * r, 2 * r + 1} <= set(ec.counts(pkg, log2n))
    big = ac.random_iq(64, 0xE000 + log2n)
    assert {32767, -32768} <= set(big[:, 0].tolist()) and {0, 16384} <= set(ec.random_window(N, 0xE100 + log2n).tolist())
    bad = ec.lane_map(pkg, synth, log2n)
    assert not bad, "\n".join(bad)


def test_2_ends(pkg, synth):
    """Spare samples of 0x7fff behind d_iq enter nothing; the sentinel behind d_out comes back untouched (on_device asserts it in
    every test); nsamp = H, the smallest call, with and without a history."""
    log2n, N, H = 9, 512, 256
    iq = ac.random_iq(3 * H, 0xE701)
    iq7 = np.concatenate([iq, np.full((7, 2), 0x7FFF, np.int16)])
    e = ec.lane_map_plan(pkg, log2n, iq)
    hist = ac.random_iq(N, 0xE702)
    bad = []
    for n in (H, 2 * H, 3 * H):
        for h in (None, hist):
            got = ec.on_device(pkg, synth, np.concatenate([iq[:n], iq7[3 * H:]]), e, h, spare=7)
            bad += ec.compare(got, ec.mirror(pkg, iq, e, h, nsamp=n), "nsamp %d" % n)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("log2n", [6, 9, 12])
def test_3_range_and_clamp(pkg, synth, log2n):
    """The inputs of the CPU tests 4 and 5: a constant -32768, alternating full scale, full-scale tones on and between bins,
    +-full-scale random and an impulse under masks of 0 .. 5/6 of the bins, and the square wave that makes the clamp work."""
    N = 1 << log2n
    bad = []
    for name, w in ec.stress_inputs(N).items():
        for k, plan in enumerate(ec.stress_plans(pkg, log2n)):
            bad += ec.check(pkg, synth, w, plan, what="%s, mask %d" % (name, k))
    w, plan = ec.square_case(pkg, log2n)
    got = ec.on_device(pkg, synth, w, plan)
    bad += ec.compare(got, ec.mirror(pkg, w, plan), "square wave")
    assert not bad, "\n".join(bad)
    print("N %d: the square wave clipped %d" % (N, got[2]))
    assert got[2] > 0


@pytest.mark.parametrize("impair", ["plain", "noise", "noise+chirp", "chirp"])
def test_4_impairments(pkg, synth, impair):
    """Plain, with a gpsbb_noise_t whose sample0 lies above 2^32, with noise and a chirp, with the chirp alone.  The handle's clip
    counters do not move; the impaired output differs from the plain one."""
    iq = (ac.random_iq(40 * 128, 0xE711).astype(np.int32) // 4).astype(np.int16)   # (room for the impairments)
    e = ec.lane_map_plan(pkg, 8, iq)
    nz = pkg._as_noise(ec.NOISE) if "noise" in impair else None
    js = ec.chirp_set(pkg) if "chirp" in impair else None
    assert ec.NOISE["sample0"] > 1 << 32
    before = clips(pkg, synth)
    hist = ac.random_iq(256, 0xE712)
    got = ec.on_device(pkg, synth, iq, e, hist, nz, js)
    bad = ec.compare(got, ec.mirror(pkg, iq, e, hist, nz, js), impair)
    assert not bad, "\n".join(bad)
    assert clips(pkg, synth) == before
    if impair != "plain":
        assert (got[0] != ec.mirror(pkg, iq, e, hist)[0]).any()


def test_5_split(pkg, synth):
    """With noise on: one call == two calls split at block k, sample k * H, sample0 advanced by as much and the history handed on:
    a k inside a workgroup's run and one at a run's boundary.  out, clipped and excised add up."""
    log2n, N, H = 8, 256, 128
    r = pkg.exc_run(log2n)
    nblk = 3 * r + 3
    iq = (ac.random_iq(nblk * H, 0xE721).astype(np.int32) // 4).astype(np.int16)   # (room for the noise)
    e = ec.lane_map_plan(pkg, log2n, iq)
    hist = ac.random_iq(N, 0xE722)
    whole = ec.on_device(pkg, synth, iq, e, hist, ec.NOISE)
    bad = ec.compare(whole, ec.mirror(pkg, iq, e, hist, ec.NOISE), "whole")
    assert whole[3] > 0
    for k in (3, r):
        nz, _ = ec.advanced(pkg, ec.NOISE, None, k * H)
        a = ec.on_device(pkg, synth, iq[:k * H], e, hist, ec.NOISE)
        b = ec.on_device(pkg, synth, iq[k * H:], e, a[1], nz)
        bad += ec.compare((np.concatenate([a[0], b[0]]), b[1], a[2] + b[2], a[3] + b[3]), whole, "split at %d" % k)
    assert not bad, "\n".join(bad)


def test_6_refusals(pkg, synth, oracle):
    """Every GPSBB_E_BADARG of the definition and the served neighbour of each; after every refusal d_out, hist_out and the counters
    are as they were and the handle still renders a block bit-exactly."""
    import torch
    L = pkg.lib()
    n = 64 * 5
    t = torch.zeros((n + 8, 2), dtype=torch.int16, device="cuda")
    o = torch.full((n + 8, 2), 0x33, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    good = pkg.exc_make(6)
    ch = pkg.synth_descriptors(1, nch=4, seed=31)[0]
    delt = 1.0 / ec.FS
    want_iq = oracle.fill_blocks(ch[None, :], delt, 1500)[0][0]
    hout = np.full((4096, 2), 0x77, np.int16)
    cl, ex = C.c_uint64(12345), C.c_uint64(54321)

    def rc(e=good, src=t.data_ptr(), dst=o.data_ptr(), nsamp=n, nz=None, js=None, null_e=False, h=None, hin=None):
        r = L.gpsbb_device_excise(synth._h if h is None else h, C.c_void_p(src) if src else None, nsamp, None if nz is None else C.byref(nz),
                                  None if js is None else C.byref(js), None if null_e else C.byref(e), None if hin is None else hin.ctypes.data,
                                  hout.ctypes.data, C.c_void_p(dst) if dst else None, C.byref(cl), C.byref(ex))
        if r != 0:
            assert (hout == 0x77).all() and (cl.value, ex.value) == (12345, 54321) and bool((o == 0x33).all())
        return r

    def still_renders():
        iq, _ = synth.fill_block(ch, delt, 1500)
        assert (iq == want_iq).all()

    def served(**kw):
        r = rc(**kw)
        ok = r == 0 and (cl.value, ex.value) != (12345, 54321) and not (hout[:64] == 0x77).all()
        hout[:] = 0x77
        cl.value, ex.value = 12345, 54321
        o.fill_(0x33)
        torch.cuda.synchronize()
        return ok

    assert served()
    still_renders()
    nz_ok = pkg.Noise(1, 5, 100.0, 1, 0)
    cw = pkg.interf_make(pkg.INTERF_CW, 0.0, 1000.0, delt=delt)
    js5 = pkg.InterfSet([cw], 0, 0)
    js5.n = 5
    w = good.window()

    def win(k, v):
        w2 = w.copy()
        w2[k] = v
        return pkg.Exc(6, 0, w2)

    cases = [("d_iq NULL", dict(src=0)), ("e NULL", dict(null_e=True)), ("d_out NULL", dict(dst=0)), ("d_iq misaligned", dict(src=t.data_ptr() + 2)),
             ("d_out misaligned", dict(dst=o.data_ptr() + 2)), ("nsamp < H", dict(nsamp=31)), ("nsamp 0", dict(nsamp=0)), ("nsamp < 0", dict(nsamp=-32)),
             ("nsamp no multiple of H", dict(nsamp=64 + 31)), ("nsamp H + 1", dict(nsamp=33)),
             ("log2n 5", dict(e=good.copy(log2n=5))), ("log2n 13", dict(e=good.copy(log2n=13))),
             ("a window entry below 0", dict(e=win(0, -1))), ("a window entry above 16384", dict(e=win(32, 16385))),
             ("halves that do not add to 16384", dict(e=win(7, int(w[7]) + 1))), ("... in the second half", dict(e=win(40, int(w[40]) - 1))),
             ("d_out == d_iq", dict(dst=t.data_ptr())), ("d_out inside d_iq", dict(dst=t.data_ptr() + 4 * (n - 1))),
             ("d_iq inside d_out", dict(src=o.data_ptr() + 4 * 31, nsamp=32)),
             ("noise sigma 0", dict(nz=pkg.Noise(1, 0, 0.0, 0, 0))), ("noise shift 8", dict(nz=pkg.Noise(1, 0, 100.0, 8, 0))),
             ("a set of 5 emitters", dict(js=js5)), ("a set's shift 8", dict(js=pkg.InterfSet([cw], 8, 0))),
             ("noise and set apart in sample0", dict(nz=nz_ok, js=pkg.InterfSet([cw], 1, 6))),
             ("noise and set apart in shift", dict(nz=nz_ok, js=pkg.InterfSet([cw], 2, 5)))]
    for what, kw in cases:
        assert rc(**kw) == BADARG, what
        still_renders()
    assert rc(h=0) == BADARG
    # the neighbours of the refusals are served
    assert served(nsamp=32) and served(nsamp=64) and served(e=good.copy(log2n=6, thr=(1 << 64) - 1)) and served(e=win(0, 0))
    big = pkg.exc_make(12)
    t12 = torch.zeros((2048, 2), dtype=torch.int16, device="cuda")
    o12 = torch.zeros((2048 + 8, 2), dtype=torch.int16, device="cuda")
    assert served(e=big, src=t12.data_ptr(), dst=o12.data_ptr(), nsamp=2048)
    assert served(dst=t.data_ptr() + 4 * 32, src=t.data_ptr(), nsamp=32)      # d_out right behind d_iq's 32 samples: no overlap
    assert served(nz=nz_ok, js=pkg.InterfSet([cw], 1, 5)) and served(nz=nz_ok) and served(js=pkg.InterfSet([cw], 1, 5))
    edge = pkg.Exc(6, 0, np.concatenate([np.full(32, 16384), np.zeros(32)]).astype(np.int16))
    assert served(e=edge)
    # hist_out, clipped and excised may be NULL; hist_out may be hist_in
    assert L.gpsbb_device_excise(synth._h, C.c_void_p(t.data_ptr()), n, None, None, C.byref(good), None, None, C.c_void_p(o.data_ptr()), None, None) == 0
    h2 = ac.random_iq(64, 0xE731)
    keep = h2.copy()
    assert L.gpsbb_device_excise(synth._h, C.c_void_p(t.data_ptr()), 32, None, None, C.byref(good), h2.ctypes.data, h2.ctypes.data, C.c_void_p(o.data_ptr()),
                                 None, None) == 0
    assert (h2[:32] == keep[32:]).all() and not h2[32:].any()
    still_renders()


def test_7_interleaved(pkg, synth):
    """Large, small, large on one handle with a device_psd, a device_fir and a device_acquire call between them: the scratch is kept
    between calls, every output == the mirror and the neighbours' results == theirs."""
    import torch
    big_iq = ac.random_iq(37 * 2048, 0xE741)
    big = ec.lane_map_plan(pkg, 12, big_iq)
    small_iq = ac.random_iq(32, 0xE742)
    small = ec.lane_map_plan(pkg, 6, small_iq)
    want_big, want_small = ec.mirror(pkg, big_iq, big), ec.mirror(pkg, small_iq, small)
    psd_iq = ac.random_iq(pc.nsamp_for(1024, 512, 9), 0xE743)
    psd = pkg.Psd(10, 512, pkg.psd_min_shift(9), pc.random_window(1024, 0xE744))
    fir_iq, fir = ac.random_iq(4096, 0xF129), fc.random_fir(pkg, 129, 16, 12, 0xF16)
    acq_iq, acq = ac.lane_map_case(pkg)
    want_psd, want_fir, want_acq = pc.mirror(pkg, psd_iq, psd), fc.mirror(pkg, fir_iq, fir), pkg.acquire_host(pkg.view_host(acq_iq), acq)
    bad = ec.compare(ec.on_device(pkg, synth, big_iq, big), want_big, "large")
    bad += pc.compare(pc.on_device(pkg, synth, psd_iq, psd), want_psd, "psd")
    bad += ec.compare(ec.on_device(pkg, synth, small_iq, small), want_small, "small")
    bad += fc.compare(fc.on_device(pkg, synth, fir_iq, fir), want_fir, "fir")
    t = torch.from_numpy(acq_iq).cuda()
    torch.cuda.synchronize()
    bad += ac.compare(synth.device_acquire(t.data_ptr(), acq_iq.shape[0], acq), None, want_acq[0], None, "acquire")
    bad += ec.compare(ec.on_device(pkg, synth, big_iq, big), want_big, "large again")
    bad += pc.compare(pc.on_device(pkg, synth, psd_iq, psd), want_psd, "psd again")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["cw", "chirp"])
def test_8_end_to_end(pkg, synth, kind):
    """acq_check's six satellites and search plan at 2.6 MS/s, 8192 samples, noise of sigma 700 at shift 1 and one emitter fused, N = 256.
    cw: a CW emitter at 317 kHz, J/S 30 dB against a gain-1.0 channel; the plan is exc_from_psd's mask (6 dB above the median bin)
    from device_psd's spectrum of the jammed view.  chirp: the README's full-band chirp (+-1.25 MHz in 0.79 ms), J/S 30 dB; the plan
    is exc_from_psd's threshold, 9 dB above the median of device_psd's spectrum of the same buffer without the emitter (a chirp fills
    every bin of an averaged spectrum and lifts its median with it; the floor is what a receiver measured before the jammer came).
    The J/S were chosen on the CPU with the mirrors (tools/exc_check.py --cpu): the search loses PRNs from 10 dB (cw) and 20 dB (chirp) on, at 30 dB all
    of them (7 findings: six PRNs wrong and the ratio test); after excision none is wrong at 10, 20, 30 and 35 dB.  Without excision
    e2e_findings on the impaired view reports at least one PRN wrong; with it, acquiring d_out + H over 7800 samples reports none.
    Every device result == its mirror."""
    import torch
    ch = ec.e2e_descriptors(pkg)
    n, H = ec.E2E_NSAMP, ec.E2E_H
    b = synth.batch(ch, 1.0 / ec.FS, n)
    try:
        b.run()
        synth.sync()
        iq = b.read()[0][0]
        d_iq = b.device_iq()
        js = ec.cw_set(pkg) if kind == "cw" else ec.sweep_set(pkg)
        cfg = ac.e2e_cfg(pkg, pkg.OUT_SC16)
        rows = synth.device_acquire(d_iq, ac.E2E_NSAMP, cfg, pkg.OUT_SC16, ec.E2E_NOISE, js)
        rows = rows[0] if isinstance(rows, tuple) else rows
        before, _, _ = ac.e2e_findings(pkg, rows, cfg, ch)
        print("%s before excision: %s" % (kind, "; ".join(before)))
        assert before
        pp = ec.e2e_psd_plan(pkg)
        spectrum, nseg = synth.device_psd(d_iq, n, pp, pkg.OUT_SC16, ec.E2E_NOISE, js if kind == "cw" else None)
        assert not pc.compare((spectrum, nseg), pc.mirror(pkg, iq, pp, 0, ec.E2E_NOISE, js if kind == "cw" else None))
        e = ec.e2e_plan(pkg, spectrum, nseg, pp, kind)
        out = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        hist, clipped, excised = synth.device_excise(d_iq, n, e, out.data_ptr(), None, ec.E2E_NOISE, js)
        bad = ec.compare((out.cpu().numpy(), hist, clipped, excised), ec.mirror(pkg, iq, e, None, ec.E2E_NOISE, js), kind)
        assert not bad, "\n".join(bad)
        rows = synth.device_acquire(out.data_ptr() + 4 * H, ac.E2E_NSAMP, cfg)
        rows = rows[0] if isinstance(rows, tuple) else rows
        after, present, absent = ac.e2e_findings(pkg, rows, cfg, ch)
        print("%s after excision: %d bins masked, thr %d, %d cells zeroed, %d clipped; present min %.2f, absent max %.2f %s" % (
            kind, int(e.bins().sum()), int(e.thr), excised, clipped, min(present.values()), max(absent.values()), "; ".join(after)))
        assert not after and excised > 0
    finally:
        b.close()
