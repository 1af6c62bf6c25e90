"""gpsbb_device_blank on the GPU (k_blank and the fold): every comparison is == on every output sample, the history handed on and
both counters against blank_host fed with view_host's output (tools/blank_check.py), on the smallest shapes at which the kernel can
go wrong — both ends of every range of the plan, sample counts around the history's length, around one and two tiles and around a
workgroup's run, with and without a history, triggers planted at tile boundaries and inside the history, the boxcar's and the
threshold's ends, every impairment, a call split inside a tile, below K and at a tile boundary, every refusal, calls interleaved
with the other calls that read device IQ — and end to end: a search that a pulsed emitter defeats finds every satellite after
blanking."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import blank_check as bc  # noqa: E402
import exc_check as ec  # noqa: E402
import psd_check as pc  # noqa: E402
from blank_check import ac, fc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1


def clips(pkg, synth):
    return synth.info(pkg.INFO_SC8_CLIPPED), synth.info(pkg.INFO_NOISE_CLIPPED)


@pytest.mark.parametrize("shape", bc.SHAPES)
def test_1_tile_map(pkg, synth, shape):
    """Random full-range int16 IQ with 32767 and -32768 in it at a threshold it passes in a few groups; nsamp 1, 2, K, K + 1, one
    below, at and one above one tile and a workgroup's run, two tiles and one; hist NULL and random."""
    Tt, r = pkg.blank_tile()
    assert (Tt, r) == (pkg.BLANK_TILE, pkg.BLANK_MIN_RUN)
    K = sum(shape) - 1
    assert {1, 2, K + 1, Tt - 1, Tt, Tt + 1, 2 * Tt + 1, r * Tt - 1, r * Tt, r * Tt + 1} | ({K} if K else set()) == set(bc.lengths(pkg, K))
    bad = bc.tile_map(pkg, synth, shape)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", [(8, 8, 8), (64, 255, 1023), (1, 0, 0)])
def test_2_planted_triggers(pkg, synth, shape):
    """Single full-scale samples on a quiet background at 0, Tt - 1, Tt, nsamp - 1 and inside the history: the one at Tt - 1 is
    staged by the first tile and blanks outputs of the second, which finds it in its halo; the one at Tt must blank nothing of the
    first tile; those in the history blank the call's first outputs.  Each blanks exactly the outputs j .. j + K."""
    L, G, hold = shape
    Tt, _ = pkg.blank_tile()
    K, n = sum(shape) - 1, 2 * Tt + 300
    b = bc.plan(pkg, shape, 1 << 30)
    bad = []
    for at, hist_at in (((0,), ()), ((Tt - 1,), ()), ((Tt,), ()), ((n - 1,), ()), ((), (K // 2,) if K else ()), ((0, Tt - 1, 2 * Tt), (0, K - 1) if K else ())):
        iq = bc.planted(n, at, 0xB300 + K)
        hist = bc.planted(max(K, 1), hist_at, 0xB301 + K)[:K]
        got = bc.on_device(pkg, synth, iq, b, hist)
        bad += bc.compare(got, bc.mirror(pkg, iq, b, hist), "at %r, in the history at %r" % (at, hist_at))
        z = bc.blanked_by(n, K, G, list(at) + [j - K for j in hist_at])
        assert got[2] == int(z.sum()) and not got[0][z].any() and (got[0][~z] == np.concatenate([hist, iq])[K - G:K - G + n][~z]).all()
    assert not bad, "\n".join(bad)


def test_3_ranges(pkg, synth):
    """A constant (-32768, -32768) with L = 64 gives s = 2^37: thr = 2^37 - 1 blanks everything, thr = 2^37 nothing; thr = 0 on
    zeros and thr = 2^64 - 1 on anything trigger nothing."""
    Tt, _ = pkg.blank_tile()
    n = Tt + 70
    full, zero, rnd = np.full((n, 2), -32768, np.int16), np.zeros((n, 2), np.int16), ac.random_iq(n, 0xB310)
    hist = np.full((63 + 16, 2), -32768, np.int16)
    bad = []
    for w, b, h, want in ((full, pkg.Blank(64, 8, 8, (1 << 37) - 1), hist, n), (full, pkg.Blank(64, 8, 8, 1 << 37), hist, 0),
                          (full, pkg.Blank(64, 8, 8, (1 << 37) - 1), None, n - 63), (zero, pkg.Blank(8, 8, 8, 0), None, 0),
                          (rnd, pkg.Blank(64, 255, 1023, (1 << 64) - 1), None, 0), (full, pkg.Blank(1, 0, 0, (1 << 64) - 1), None, 0),
                          (full, pkg.Blank(1, 0, 0, (1 << 31) - 1), None, n), (full, pkg.Blank(1, 0, 0, 1 << 31), None, 0)):
        got = bc.on_device(pkg, synth, w, b, h)
        bad += bc.compare(got, bc.mirror(pkg, w, b, h), "thr %d L %d" % (b.thr, b.win))
        assert got[3] == want, (b.thr, b.win)
    assert not bad, "\n".join(bad)


def test_4_ends(pkg, synth):
    """Spare samples of 0x7fff behind d_iq enter nothing; the sentinel behind d_out comes back untouched (on_device asserts it in
    every test)."""
    Tt, _ = pkg.blank_tile()
    iq = (ac.random_iq(Tt + 5, 0xB320).astype(np.int32) // 8).astype(np.int16)
    b = bc.plan(pkg, (8, 8, 8), bc.random_thr((8, 8, 8), iq))
    hist = bc.random_hist(23, 0xB321)
    bad = []
    for n in (1, 5, Tt - 1, Tt, Tt + 5):
        for h in (None, hist):
            got = bc.on_device(pkg, synth, np.concatenate([iq[:n], np.full((7, 2), 0x7FFF, np.int16)]), b, h, spare=7)
            bad += bc.compare(got, bc.mirror(pkg, iq, b, h, nsamp=n), "nsamp %d" % n)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("impair", ["plain", "noise", "noise+chirp", "chirp"])
def test_5_impairments(pkg, synth, impair):
    """Plain, with a gpsbb_noise_t whose sample0 lies above 2^32, with noise and a chirp, with the chirp alone.  The handle's clip
    counters do not move; the impaired output differs from the plain one."""
    Tt, _ = pkg.blank_tile()
    iq = (ac.random_iq(Tt + 1000, 0xB330).astype(np.int32) // 4).astype(np.int16)   # (room for the impairments)
    nz = pkg._as_noise(bc.NOISE) if "noise" in impair else None
    js = fc.chirp_set(pkg) if "chirp" in impair else None
    assert bc.NOISE["sample0"] > 1 << 32
    b = bc.plan(pkg, (8, 8, 8), bc.random_thr((8, 8, 8), pkg.view_host(iq, pkg.OUT_SC16, nz, interf=js)))
    before = clips(pkg, synth)
    hist = bc.random_hist(23, 0xB331)
    got = bc.on_device(pkg, synth, iq, b, hist, nz, js)
    bad = bc.compare(got, bc.mirror(pkg, iq, b, hist, nz, js), impair)
    assert not bad, "\n".join(bad)
    assert clips(pkg, synth) == before and got[3] > 0 and 0 < got[2] < iq.shape[0]
    if impair != "plain":
        assert (got[0] != bc.mirror(pkg, iq, b, hist)[0]).any()


def test_6_split(pkg, synth):
    """With noise on: one call == two calls split at sample k, sample0 advanced by as much and the history handed on: an odd k
    inside a tile, a k below K and a tile boundary.  out, blanked and triggers add up."""
    Tt, _ = pkg.blank_tile()
    shape = (16, 30, 100)
    K, n = sum(shape) - 1, 2 * Tt + 501
    iq = (ac.random_iq(n, 0xB340).astype(np.int32) // 4).astype(np.int16)   # (room for the noise)
    b = bc.plan(pkg, shape, bc.random_thr(shape, pkg.view_host(iq, pkg.OUT_SC16, bc.NOISE)))
    hist = bc.random_hist(K, 0xB341)
    whole = bc.on_device(pkg, synth, iq, b, hist, bc.NOISE)
    bad = bc.compare(whole, bc.mirror(pkg, iq, b, hist, bc.NOISE), "whole")
    assert whole[3] > 0 and 0 < whole[2] < n
    assert 37 < K < 1531 < Tt
    for k in (1531, 37, Tt, n - 1):
        nz, _ = fc.advanced(pkg, bc.NOISE, None, k)
        a = bc.on_device(pkg, synth, iq[:k], b, hist, bc.NOISE)
        c = bc.on_device(pkg, synth, iq[k:], b, a[1], nz)
        bad += bc.compare((np.concatenate([a[0], c[0]]), c[1], a[2] + c[2], a[3] + c[3]), whole, "split at %d" % k)
    assert not bad, "\n".join(bad)


def test_7_refusals(pkg, synth, oracle):
    """Every GPSBB_E_BADARG of the definition and the served neighbour of each; after every refusal d_out, hist_out and the counters
    are as they were and the handle still renders a block bit-exactly."""
    import torch
    L = pkg.lib()
    n = 300
    t = torch.zeros((n + 8, 2), dtype=torch.int16, device="cuda")
    o = torch.full((n + 8, 2), 0x33, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    good = pkg.Blank(8, 8, 8, 1000)
    ch = pkg.synth_descriptors(1, nch=4, seed=31)[0]
    delt = 1.0 / bc.FS
    want_iq = oracle.fill_blocks(ch[None, :], delt, 1500)[0][0]
    hout = np.full((pkg.BLANK_MAX_HIST, 2), 0x77, np.int16)
    bl, tr = C.c_uint64(12345), C.c_uint64(54321)

    def rc(b=good, src=t.data_ptr(), dst=o.data_ptr(), nsamp=n, nz=None, js=None, null_b=False, h=None, hin=None):
        r = L.gpsbb_device_blank(synth._h if h is None else h, C.c_void_p(src) if src else None, nsamp, None if nz is None else C.byref(nz),
                                 None if js is None else C.byref(js), None if null_b else C.byref(b), None if hin is None else hin.ctypes.data,
                                 hout.ctypes.data, C.c_void_p(dst) if dst else None, C.byref(bl), C.byref(tr))
        if r != 0:
            assert (hout == 0x77).all() and (bl.value, tr.value) == (12345, 54321) and bool((o == 0x33).all())
        return r

    def still_renders():
        iq, _ = synth.fill_block(ch, delt, 1500)
        assert (iq == want_iq).all()

    def served(**kw):
        r = rc(**kw)
        K = kw.get("b", good).hist()
        ok = r == 0 and (bl.value, tr.value) == (0, 0) and not hout[:K].any() and (hout[K:] == 0x77).all()
        hout[:] = 0x77
        bl.value, tr.value = 12345, 54321
        o.fill_(0x33)
        torch.cuda.synchronize()
        return ok

    assert served()
    still_renders()
    nz_ok = pkg.Noise(1, 5, 100.0, 1, 0)
    cw = pkg.interf_make(pkg.INTERF_CW, 0.0, 1000.0, delt=delt)
    js5 = pkg.InterfSet([cw], 0, 0)
    js5.n = 5
    cases = [("d_iq NULL", dict(src=0)), ("b NULL", dict(null_b=True)), ("d_out NULL", dict(dst=0)), ("d_iq misaligned", dict(src=t.data_ptr() + 2)),
             ("d_out misaligned", dict(dst=o.data_ptr() + 2)), ("nsamp 0", dict(nsamp=0)), ("nsamp < 0", dict(nsamp=-5)),
             ("win 0", dict(b=good.copy(win=0))), ("win 65", dict(b=good.copy(win=65))), ("pre -1", dict(b=good.copy(pre=-1))),
             ("pre 256", dict(b=good.copy(pre=256))), ("hold -1", dict(b=good.copy(hold=-1))), ("hold 1024", dict(b=good.copy(hold=1024))),
             ("_pad 1", dict(b=good.copy(_pad=1))),
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
    # the neighbours of the refusals are served (zeros in, a threshold of 1000: nothing triggers, the history handed on is zeros)
    assert served(nsamp=1) and served(b=good.copy(win=1)) and served(b=good.copy(win=64)) and served(b=good.copy(pre=0)) and served(b=good.copy(pre=255))
    assert served(b=good.copy(hold=0)) and served(b=good.copy(hold=1023)) and served(b=good.copy(thr=(1 << 64) - 1)) and served(b=pkg.Blank(1, 0, 0, 5))
    assert served(dst=t.data_ptr() + 4 * 32, src=t.data_ptr(), nsamp=32)      # d_out right behind d_iq's 32 samples: no overlap
    for kw in (dict(nz=nz_ok, js=pkg.InterfSet([cw], 1, 5)), dict(nz=nz_ok), dict(js=pkg.InterfSet([cw], 1, 5))):
        assert rc(**kw) == 0 and hout[:23].any() and (hout[23:] == 0x77).all()      # (an impaired history is not zeros)
        hout[:] = 0x77
    # hist_out, blanked and triggers may be NULL; hist_out may be hist_in
    assert L.gpsbb_device_blank(synth._h, C.c_void_p(t.data_ptr()), n, None, None, C.byref(good), None, None, C.c_void_p(o.data_ptr()), None, None) == 0
    h2 = bc.random_hist(23, 0xB351)
    keep = h2.copy()
    assert L.gpsbb_device_blank(synth._h, C.c_void_p(t.data_ptr()), 10, None, None, C.byref(good), h2.ctypes.data, h2.ctypes.data, C.c_void_p(o.data_ptr()),
                                None, None) == 0
    assert (h2[:13] == keep[10:]).all() and not h2[13:].any()
    still_renders()


def test_8_interleaved(pkg, synth):
    """Large, small, large on one handle with a device_fir, a device_psd, a device_excise and a device_acquire call between them:
    the scratch is kept between calls, every output == the mirror and the neighbours' results == what they give alone."""
    import torch
    Tt, _ = pkg.blank_tile()
    big_iq, small_iq = ac.random_iq(2 * Tt + 77, 0xB361), ac.random_iq(9, 0xB362)
    big, small = bc.plan(pkg, (64, 255, 1023), bc.random_thr((64, 255, 1023), big_iq)), bc.plan(pkg, (2, 1, 3), bc.random_thr((2, 1, 3), small_iq))
    want_big, want_small = bc.mirror(pkg, big_iq, big), bc.mirror(pkg, small_iq, small)
    psd_iq = ac.random_iq(pc.nsamp_for(1024, 512, 9), 0xE743)
    psd = pkg.Psd(10, 512, pkg.psd_min_shift(9), pc.random_window(1024, 0xE744))
    fir_iq, fir = ac.random_iq(4096, 0xF129), fc.random_fir(pkg, 129, 16, 12, 0xF16)
    exc_iq = ac.random_iq(5 * 128, 0xE745)
    exc = ec.lane_map_plan(pkg, 8, exc_iq)
    acq_iq, acq = ac.lane_map_case(pkg)
    want_psd, want_fir, want_exc = pc.mirror(pkg, psd_iq, psd), fc.mirror(pkg, fir_iq, fir), ec.mirror(pkg, exc_iq, exc)
    want_acq = pkg.acquire_host(pkg.view_host(acq_iq), acq)
    t = torch.from_numpy(acq_iq).cuda()
    torch.cuda.synchronize()
    # alone, before the blanker's scratch exists
    bad = fc.compare(fc.on_device(pkg, synth, fir_iq, fir), want_fir, "fir alone")
    bad += pc.compare(pc.on_device(pkg, synth, psd_iq, psd), want_psd, "psd alone")
    bad += ec.compare(ec.on_device(pkg, synth, exc_iq, exc), want_exc, "excise alone")
    bad += ac.compare(synth.device_acquire(t.data_ptr(), acq_iq.shape[0], acq), None, want_acq[0], None, "acquire alone")
    bad += bc.compare(bc.on_device(pkg, synth, big_iq, big), want_big, "large")
    bad += fc.compare(fc.on_device(pkg, synth, fir_iq, fir), want_fir, "fir")
    bad += bc.compare(bc.on_device(pkg, synth, small_iq, small), want_small, "small")
    bad += pc.compare(pc.on_device(pkg, synth, psd_iq, psd), want_psd, "psd")
    bad += ec.compare(ec.on_device(pkg, synth, exc_iq, exc), want_exc, "excise")
    bad += bc.compare(bc.on_device(pkg, synth, big_iq, big), want_big, "large again")
    bad += ac.compare(synth.device_acquire(t.data_ptr(), acq_iq.shape[0], acq), None, want_acq[0], None, "acquire")
    bad += bc.compare(bc.on_device(pkg, synth, small_iq, small), want_small, "small again")
    assert not bad, "\n".join(bad)


def test_9_end_to_end(pkg, synth):
    """exc_check's six satellites and search plan at 2.6 MS/s, 8192 samples, noise of sigma 700 at shift 1 and a CW emitter at 317 kHz
    pulsed with period 0.7 ms and duty 0.10 at J/S 40 dB, fused.  The plan is blank_from_level's, 6 dB above the lower median of
    device_level's levels of the same buffer with the emitter in it over blocks of 64 samples, L = G = hold = 8.  Without blanking
    e2e_findings on the impaired view reports at least one PRN wrong; with it, acquiring d_out + G over 7800 samples reports none,
    at most 12 % of the samples are blanked and at most 0.1 % of the quiet buffer under the same plan.  On the mirrors
    (tools/blank_check.py --cpu): 6 findings before, none after, 820 of 8192 blanked, 0 of the quiet buffer.  Every device result ==
    its mirror."""
    import torch
    ch = ec.e2e_descriptors(pkg)
    n, G = bc.E2E_NSAMP, bc.E2E_SHAPE[1]
    bt = synth.batch(ch, 1.0 / bc.FS, n)
    try:
        bt.run()
        synth.sync()
        iq = bt.read()[0][0]
        d_iq = bt.device_iq()
        js = bc.pulsed_set(pkg)
        cfg = ac.e2e_cfg(pkg, pkg.OUT_SC16)
        rows = synth.device_acquire(d_iq, ac.E2E_NSAMP, cfg, pkg.OUT_SC16, bc.E2E_NOISE, js)
        before, _, _ = ac.e2e_findings(pkg, rows, cfg, ch)
        print("before blanking: %s" % "; ".join(before))
        assert before
        levels = synth.device_level(d_iq, n // bc.E2E_BLOCK, bc.E2E_BLOCK, bc.E2E_NOISE, js)
        want_levels = pkg.level_host(iq.reshape(n // bc.E2E_BLOCK, bc.E2E_BLOCK, 2), bc.E2E_NOISE, js)
        assert all((levels[f] == want_levels[f]).all() for f in ("n", "sumsq", "hist"))
        b = bc.e2e_plan(pkg, levels)
        out = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        hist, blanked, triggers = synth.device_blank(d_iq, n, b, out.data_ptr(), None, bc.E2E_NOISE, js)
        bad = bc.compare((out.cpu().numpy(), hist, blanked, triggers), bc.mirror(pkg, iq, b, None, bc.E2E_NOISE, js), "pulsed")
        assert not bad, "\n".join(bad)
        rows = synth.device_acquire(out.data_ptr() + 4 * G, ac.E2E_NSAMP, cfg)
        after, present, absent = ac.e2e_findings(pkg, rows, cfg, ch)
        quiet = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        _, quiet_blanked, _ = synth.device_blank(d_iq, n, b, quiet.data_ptr(), None, bc.E2E_NOISE)
        assert quiet_blanked == bc.mirror(pkg, iq, b, None, bc.E2E_NOISE)[2]
        print("after blanking: thr %d, %d triggers, %d of %d blanked (%.1f %%), %d of the quiet buffer; present min %.2f, absent max %.2f %s" % (
            int(b.thr), triggers, blanked, n, 100.0 * blanked / n, quiet_blanked, min(present.values()), max(absent.values()), "; ".join(after)))
        assert not after
        budget = bc.e2e_budget(blanked, quiet_blanked)
        assert not budget, "\n".join(budget)
    finally:
        bt.close()
