"""gpsbb_device_psd against the numpy restatement (psd_host over view_host): the cases and the comparison that tests/test_psd.py
and tests/test_psd_gpu.py share.  Every comparison is == on integers: every bin and the segment count.  Run as a script it checks
the cases on the GPU and prints what it compared; --cpu runs the end-to-end cases (a CW emitter on a bin centre, a chirp over a
band, a stop-band tone through the front-end filter, the sum of the bins against the level) with the CPU oracle's render and the
numpy mirrors only, and prints the figures the GPU test asserts:

    python tools/psd_check.py [--cpu]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402
import fir_check as fc  # noqa: E402
import track_check as tc  # noqa: E402

FS = ac.FS
NOISE = ac.NOISE
LOG2NS = (6, 7, 8, 9, 10, 11, 12)


def hops(N):
    return (1, N // 2, N, N + 3)


def counts(pkg, log2n):
    """the segment counts of the stage and lane map: 1, 2, 5, and one below, at and one above one and two workgroup runs"""
    r = pkg.psd_run(log2n)
    return sorted({1, 2, 5, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1} - {0})


def nsamp_for(N, hop, nseg):
    return N + (nseg - 1) * hop


def random_window(N, seed):
    """random int16 over the whole range, -32768 among them"""
    w = np.random.default_rng(seed).integers(-32768, 32768, N, dtype=np.int64).astype(np.int16)
    w[N // 3] = -32768
    w[0] = 32767
    return w


def plan(pkg, log2n, hop, nseg, win, shift=None):
    return pkg.Psd(log2n, hop, pkg.psd_min_shift(nseg) if shift is None else shift, win)


def on_device(pkg, synth, iq, psd, view=0, noise=None, interf=None, nsamp=None, spare=0):
    """the call on host array iq [n, 2] through a device buffer -> (psd uint64 [N], nseg)"""
    import torch
    n = iq.shape[0] - spare if nsamp is None else nsamp
    t = torch.from_numpy(np.ascontiguousarray(iq, np.int16)).cuda()
    torch.cuda.synchronize()
    return synth.device_psd(t.data_ptr(), n, psd, view, noise, interf)


def mirror(pkg, iq, psd, view=0, noise=None, interf=None, nsamp=None):
    n = iq.shape[0] if nsamp is None else nsamp
    return pkg.psd_host(pkg.view_host(iq[:n], view, noise, interf=interf), psd, view)


def compare(got, want, what=""):
    """findings (strings) of (psd, nseg) against the same from the mirror"""
    bad = []
    (gp, gn), (wp, wn) = got, want
    if gn != wn:
        bad.append("%s nseg: %d, want %d" % (what, gn, wn))
    if gp.shape != wp.shape or not (gp == wp).all():
        w = np.flatnonzero(gp != wp) if gp.shape == wp.shape else []
        bad.append("%s psd: %d bins differ, first %s" % (what, len(w), "%d: %d, want %d" % (w[0], gp[w[0]], wp[w[0]]) if len(w) else
                                                        "shape %r / %r" % (gp.shape, wp.shape)))
    return bad


def check(pkg, synth, iq, psd, view=0, noise=None, interf=None, nsamp=None, what=""):
    return compare(on_device(pkg, synth, iq, psd, view, noise, interf, nsamp), mirror(pkg, iq, psd, view, noise, interf, nsamp), what)


def lane_map(pkg, synth, log2n):
    """findings of every hop and count at one N, on one random buffer under one random window"""
    N = 1 << log2n
    cs = counts(pkg, log2n)
    iq = ac.random_iq(nsamp_for(N, N + 3, cs[-1]), 0x9500 + log2n)
    win = random_window(N, 0x9D00 + log2n)
    bad = []
    for hop in hops(N):
        for nseg in cs:
            n = nsamp_for(N, hop, nseg)
            bad += check(pkg, synth, iq, plan(pkg, log2n, hop, nseg, win), nsamp=n, what="N %d hop %d nseg %d" % (N, hop, nseg))
    return bad


def chirp_set(pkg, fs=FS):
    return fc.chirp_set(pkg, fs)


def advanced(pkg, noise, interf, n):
    return fc.advanced(pkg, noise, interf, n)


# ---- end to end: what the spectrum is for ----

E2E_LOG2N, E2E_N = 10, 1024
E2E_NSAMP = E2E_N + 31 * (E2E_N // 2)      # 32 Hann segments of six satellites at 2.6 MS/s
E2E_K0 = 100                               # the CW emitter's bin: +-100 * 2.6e6 / 1024 = +-253.9 kHz
E2E_CW_JS_DB = 20.0
E2E_CHIRP = (300e3, 700e3, 10.0)           # f0, f1, J/S in dB
E2E_TONE_JS_DB = 34.5                      # the stop-band tone: amplitude 512 * 10^(34.5 / 20) = 27 000, below sat16's clamp
E2E_FIR_NSAMP_IN = 4 * (E2E_N + 15 * (E2E_N // 2))   # 16 Hann segments after the filter, 10.4 MS/s before
E2E_MARGIN_DB = 0.25                       # see stop_band_bin: the mirror is within 0.02 dB


def e2e_descriptors(pkg):
    return tc.e2e_descriptors(pkg)


def hann_plan(pkg, nsamp):
    return pkg.psd_make(E2E_LOG2N, nsamp, 0, pkg.PSD_HANN)


def cw_set(pkg, k0, js_db=E2E_CW_JS_DB, fs=FS):
    """one CW emitter on the centre of bin k0 (negative: below the carrier) of an N = 1024 transform"""
    return pkg.InterfSet([pkg.interf_make(pkg.INTERF_CW, js_db, k0 * fs / E2E_N, delt=1.0 / fs)], 0, 0)


def band_set(pkg, fs=FS):
    f0, f1, js = E2E_CHIRP
    return pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, js, f0, f1, 997.0 / fs, delt=1.0 / fs)], 0, 0)


def band_bins(fs=FS):
    f0, f1, _ = E2E_CHIRP
    return int(np.ceil(f0 * E2E_N / fs)), int(np.floor(f1 * E2E_N / fs))


def band_share(p, fs=FS):
    k0, k1 = band_bins(fs)
    p = p.astype(np.float64)
    return p[k0:k1 + 1].sum() / p.sum()


def predicted_share(pkg, ch, js_db):
    """the emitter's share of the whole power from the gains alone: an emitter of level g has the power of a channel of gain g"""
    pj = 10.0 ** (js_db / 10.0)
    ps = float((ch["gain"].astype(np.float64) ** 2).sum())
    return pj / (pj + ps)


def stop_band_bin(pkg, fir):
    """(the bin of an N = 1024 transform at the input rate whose frequency the filter takes down by nearest to 40 dB, on the rising
    side of its stop band's edge; the response there in dB; the bin it aliases to after decimation)"""
    f, db = fc.response_db(fir, E2E_N)
    k = int(np.argmin(np.abs(db[:E2E_N // 4] + 40.0)))
    return k, float(db[k]), (k * int(fir.decim)) % E2E_N


def bin_db(p, psd, nseg, k):
    """the power of bin k in dB, segments and shift taken out"""
    return 10.0 * np.log10(float(p[k]) * 4.0 ** int(psd.shift) / nseg)


def e2e_cpu(pkg):
    """the end-to-end cases on the CPU oracle's render with the mirrors alone -> findings; prints the figures"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_binding as ob
    bad = []
    ch = e2e_descriptors(pkg)
    iq = ob.Oracle().fill_blocks(ch, 1.0 / FS, E2E_NSAMP)[0][0]
    p = hann_plan(pkg, E2E_NSAMP)
    for k0 in (E2E_K0, -E2E_K0):
        got, _ = mirror(pkg, iq, p, interf=cw_set(pkg, k0))
        print("CW at bin %d: largest bin %d" % (k0, int(np.argmax(got))))
        if int(np.argmax(got)) != k0 % E2E_N:
            bad.append("CW at bin %d: largest bin %d" % (k0, int(np.argmax(got))))
    plain, nseg = mirror(pkg, iq, p)
    band, _ = mirror(pkg, iq, p, interf=band_set(pkg))
    gain, want = band_share(band) - band_share(plain), predicted_share(pkg, ch, E2E_CHIRP[2])
    print("chirp: share in band %.4f, without %.4f, predicted %.4f" % (band_share(band), band_share(plain), want))
    if not (gain > 0 and gain >= 0.5 * want):
        bad.append("chirp: the band gained %.4f of the power, predicted %.4f" % (gain, want))
    lv = pkg.level_host(iq)
    rect = pkg.psd_make(E2E_LOG2N, E2E_NSAMP)
    pr, nr = mirror(pkg, iq, rect)
    n_used = nr * E2E_N
    exact = float((iq[:n_used].astype(np.int64) ** 2).sum()) / n_used
    est = float(pr.astype(np.float64).sum()) * pkg.psd_scale(rect, nr)
    print("sum of the bins: %.6g against the mean square %.6g (%.2e); level_host's %.6g" % (est, exact, est / exact - 1.0,
                                                                                           float(lv["sumsq"].sum()) / float(lv["n"].sum())))
    if abs(est / exact - 1.0) > 1e-4:
        bad.append("sum of the bins off by %.2e" % (est / exact - 1.0))
    # the stop-band tone through the filter
    fir = fc.e2e_fir(pkg)
    k, db, kout = stop_band_bin(pkg, fir)
    js = cw_set(pkg, k, E2E_TONE_JS_DB, fc.FS_IN)
    w = pkg.view_host(np.zeros((E2E_FIR_NSAMP_IN, 2), np.int16), interf=js).astype(np.int16)
    y, _, clipped = pkg.fir_host(w, fir)
    pin, pout = hann_plan(pkg, w.shape[0]), hann_plan(pkg, y.shape[0])
    (a, na), (b, nb) = pkg.psd_host(w, pin), pkg.psd_host(y, pout)
    drop = bin_db(a, pin, na, k) - bin_db(b, pout, nb, kout)
    print("stop band: bin %d (%.1f kHz), response %.3f dB, aliased to bin %d, drop %.3f dB, off by %.4f dB, clipped %d" % (
        k, k * fc.FS_IN / E2E_N / 1e3, db, kout, drop, drop + db, clipped))
    if abs(drop + db) > E2E_MARGIN_DB:
        bad.append("stop band: drop %.3f dB against the response %.3f dB" % (drop, db))
    return bad


def main():
    sys.path.insert(0, ROOT)
    cpu = "--cpu" in sys.argv[1:]
    if not cpu:
        try:
            import torch  # noqa: F401  (one HIP runtime for torch and libgpsbb)
        except Exception:
            pass
    from __graft_entry__ import load_package
    pkg = load_package()
    bad = []
    if cpu:
        bad = e2e_cpu(pkg)
    else:
        with pkg.Synth(0) as s:
            for log2n in LOG2NS:
                bad += lane_map(pkg, s, log2n)
                print("N %d: hops %s, segments %s" % (1 << log2n, list(hops(1 << log2n)), counts(pkg, log2n)), flush=True)
            iq = (ac.random_iq(256 + 40 * 128, 0x95F).astype(np.int32) // 4).astype(np.int16)
            p = pkg.psd_make(8, iq.shape[0], 0, pkg.PSD_HANN)
            for view in (pkg.OUT_SC16, pkg.OUT_SC8(3), pkg.OUT_SC1):
                for what, nz, js in (("plain", None, None), ("noise", NOISE, None), ("noise + chirp", NOISE, chirp_set(pkg)), ("chirp", None, chirp_set(pkg))):
                    bad += check(pkg, s, iq, p, view, nz, js, what="view 0x%x %s" % (view, what))
                print("view 0x%x: plain, noise, noise + chirp, chirp" % view, flush=True)
    if bad:
        print("\n".join(bad))
        return 1
    print("the spectrum is bit-exact against the numpy mirror" if not cpu else "the end-to-end figures hold on the mirror")
    return 0


if __name__ == "__main__":
    sys.exit(main())
