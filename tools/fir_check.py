"""gpsbb_device_fir against the numpy restatement (fir_host over view_host): the cases and the comparison that tests/test_fir.py
and tests/test_fir_gpu.py share.  Every comparison is == on integers: every output sample, the history handed on, the clip count.
Run as a script it checks the cases on the GPU and prints what it compared; --cpu runs the end-to-end case (six satellites
rendered at 10.4 MS/s, filtered and decimated to 2.6 MS/s, acquired, tracked, their data bits read back) with the CPU oracle's
render and the numpy mirrors only:

    python tools/fir_check.py [--cpu]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402
import track_check as tc  # noqa: E402

FS = ac.FS
NOISE = ac.NOISE
SHAPES = ((1, 1), (2, 1), (33, 4), (128, 16), (129, 16), (5, 3), (64, 7))   # (T, D): odd D, even T, both ends of both ranges


def outputs(pkg):
    """the output counts of the lane and tile map: around one tile, and a third tile that is ragged"""
    t = pkg.FIR_TILE
    return (1, 2, t - 1, t, t + 1, 2 * t + 3)


def random_fir(pkg, T, D, shift, seed, budget=65535):
    """random taps of both signs with the sum of |h| exactly `budget` (or 32767 * T where that is less)"""
    rng = np.random.default_rng(seed)
    w = rng.random(T) + 0.05
    h = np.floor(w / w.sum() * min(budget, 32767 * T)).astype(np.int64)
    h = np.minimum(h, 32767)
    k = 0
    while h.sum() < min(budget, 32767 * T):
        if h[k % T] < 32767:
            h[k % T] += 1
        k += 1
    h *= rng.choice([-1, 1], T)
    return pkg.Fir([int(v) for v in h], D, shift)


def random_hist(T, seed):
    return ac.random_iq(max(T - 1, 5), seed)[:T - 1] if T > 1 else np.zeros((0, 2), np.int16)


def on_device(pkg, synth, iq, fir, hist=None, noise=None, interf=None, nsamp=None, spare=0, canary=3):
    """the call on host array iq [n, 2] through device buffers -> (y, hist_out, clipped).  The output buffer is `canary` samples
    longer than the call may write, filled with 0x5a5a before: they must come back as they were"""
    import torch
    n = iq.shape[0] - spare if nsamp is None else nsamp
    t = torch.from_numpy(np.ascontiguousarray(iq, np.int16)).cuda()
    m = n // int(fir.decim)
    out = torch.full((m + canary, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    hout, clipped = synth.device_fir(t.data_ptr(), n, fir, out.data_ptr(), hist, noise, interf)
    got = out.cpu().numpy()
    assert (got[m:] == 0x5A5A).all(), "the call wrote behind its output"
    return got[:m], hout, clipped


def mirror(pkg, iq, fir, hist=None, noise=None, interf=None, nsamp=None):
    n = iq.shape[0] if nsamp is None else nsamp
    return pkg.fir_host(pkg.view_host(iq[:n], pkg.OUT_SC16, noise, interf=interf), fir, hist)


def compare(got, want, what=""):
    """findings (strings) of (y, hist_out, clipped) against the same from the mirror"""
    bad = []
    (gy, gh, gc), (wy, wh, wc) = got, want
    if gy.shape != wy.shape or not (gy == wy).all():
        w = np.argwhere(gy != wy) if gy.shape == wy.shape else []
        bad.append("%s y: %d components differ, first (m, c) %s" % (what, len(w), w[0].tolist() if len(w) else "shape %r / %r" % (gy.shape, wy.shape)))
    if gh.shape != wh.shape or not (gh == wh).all():
        w = np.argwhere(gh != wh) if gh.shape == wh.shape else []
        bad.append("%s history: %d components differ, first %s" % (what, len(w), w[0].tolist() if len(w) else "shape"))
    if gc != wc:
        bad.append("%s clipped: %d, want %d" % (what, gc, wc))
    return bad


def check(pkg, synth, iq, fir, hist=None, noise=None, interf=None, what=""):
    return compare(on_device(pkg, synth, iq, fir, hist, noise, interf), mirror(pkg, iq, fir, hist, noise, interf), what)


def chirp_set(pkg, fs=FS):
    delt = 1.0 / fs
    return pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -0.2 * fs, 0.27 * fs, 301 * delt, delt=delt)], NOISE["shift"], NOISE["sample0"])


def advanced(pkg, noise, interf, n):
    """noise and set with sample0 moved on by n: what a later call of a split gets"""
    nz = None
    if noise is not None:
        nz = dict(noise)
        nz["sample0"] = noise["sample0"] + n
    js = None
    if interf is not None:
        js = pkg.InterfSet([interf.e[k] for k in range(interf.n)], interf.shift, interf.sample0 + n)
    return nz, js


# ---- the taps' frequency response, from the taps alone ----

def response_db(fir, nfft=1 << 16):
    """(f in cycles per input sample, 20 log10 |H(f)| relative to DC) on nfft / 2 + 1 points"""
    h = fir.taps().astype(np.float64)
    H = np.abs(np.fft.rfft(h, nfft)) / abs(h.sum())
    return np.arange(H.size) / float(nfft), 20.0 * np.log10(np.maximum(H, 1e-12))


def design_numpy(T, D, cutoff, atten_db):
    """gpsbb_fir_make's g[k] * 2^15 with numpy's own window and sinc"""
    beta = 0.1102 * (atten_db - 8.7) if atten_db > 50 else (0.5842 * (atten_db - 21) ** 0.4 + 0.07886 * (atten_db - 21) if atten_db >= 21 else 0.0)
    fc = cutoff * 0.5 / D
    k = np.arange(T) - (T - 1) / 2.0
    g = 2 * fc * np.sinc(2 * fc * k) * np.kaiser(T, beta)
    return g / g.sum() * 32768.0


# ---- end to end: rendered at four times the rate, filtered, decimated, acquired, tracked ----

E2E_D, E2E_T = 4, 33
E2E_NSAMP_IN = tc.E2E_NSAMP * E2E_D      # 5 200 000 samples at 10.4 MS/s
FS_IN = FS * E2E_D


def e2e_fir(pkg):
    return pkg.fir_make(E2E_T, E2E_D)


def e2e_first_wraps(pkg, ch):
    """per present PRN the output lag of its first code wrap before the filter's delay, (1023 - code_phase) / (f_code * delt) at
    2.6 MS/s.  Output m is centred on input m * D + (D - 1) - (T - 1) / 2 = 4 m - 13: the filter delays the signal by 13 input
    samples, 3.25 output samples or 1.28 chips (the issue's 3.1 samples and 1.2 chips, to its rounding).  A wrap that lies more
    than 4 samples before lag 2600 is still the stream's first, and no epoch numbering moves"""
    return [(1023.0 - float(ch[0, p - 1]["code_phase"])) / (float(ch[0, p - 1]["f_code"]) / FS) for p in tc.E2E_PRESENT]


def e2e_chain_host(pkg, y):
    """the existing chain on the decimated stream y [1 300 000, 2] with the numpy mirrors -> the records per PRN"""
    acq = tc.e2e_acq_cfg(pkg, pkg.OUT_SC16)
    rows, _ = pkg.acquire_host(pkg.view_host(y[:tc.E2E_ACQ_NSAMP]), acq)
    st = tc.e2e_seeds(pkg, rows, acq)
    _, recs = pkg.track_host(pkg.view_host(y), tc.e2e_trk_cfg(pkg), st)
    return recs


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
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_binding as ob
        ch = tc.e2e_descriptors(pkg)
        iq = ob.Oracle().fill_blocks(ch, 1.0 / FS_IN, E2E_NSAMP_IN)[0][0]
        y, _, clipped = pkg.fir_host(pkg.view_host(iq), e2e_fir(pkg))
        print("filtered: %d samples, clipped %d, first wraps at output lags %s" % (y.shape[0], clipped, ["%.0f" % v for v in e2e_first_wraps(pkg, ch)]), flush=True)
        bad, (min_pi, max_pq) = tc.e2e_findings(pkg, ch, e2e_chain_host(pkg, y))
        print("min |P.i| %.3g, max |P.q| %.3g after epoch %d" % (min_pi, max_pq, tc.E2E_SKIP))
    else:
        with pkg.Synth(0) as s:
            for T, D in SHAPES:
                for M in outputs(pkg):
                    iq = ac.random_iq(max(M * D, 5), 0xF100 + T)[:M * D]
                    fir = random_fir(pkg, T, D, 15, T * 31 + D)
                    bad += check(pkg, s, iq, fir, None, what="T %d D %d M %d" % (T, D, M))
                    bad += check(pkg, s, iq, fir, random_hist(T, 0xF1), what="T %d D %d M %d with history" % (T, D, M))
                print("T %d D %d: %s outputs, with and without history" % (T, D, list(outputs(pkg))), flush=True)
            iq = ac.random_iq(4 * 700, 0xF2)
            fir = pkg.fir_make(33, 4)
            for what, nz, js in (("plain", None, None), ("noise", NOISE, None), ("noise + chirp", NOISE, chirp_set(pkg)), ("chirp", None, chirp_set(pkg))):
                bad += check(pkg, s, iq, fir, None, nz, js, what=what)
                print("(33, 4) %s" % what, flush=True)
    if bad:
        print("\n".join(bad))
        return 1
    print("the filter is bit-exact against the numpy mirror" if not cpu else "all six satellites hold through the filter")
    return 0


if __name__ == "__main__":
    sys.exit(main())
