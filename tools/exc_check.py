"""gpsbb_device_excise against the numpy restatement (excise_host over view_host): the cases and the comparison that
tests/test_excise.py and tests/test_excise_gpu.py share.  Every comparison is == on integers: every output sample, the history
handed on and both counters.  Run as a script it checks the cases on the GPU and prints what it compared; --cpu runs the
end-to-end cases (six satellites under noise and a CW emitter, then a full-band chirp, acquired before and after excision) with the
CPU oracle's render and the numpy mirrors only, and prints the figures the GPU test asserts:

    python tools/exc_check.py [--cpu]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402
import fir_check as fc  # noqa: E402

FS = ac.FS
NOISE = ac.NOISE
LOG2NS = (6, 7, 8, 9, 10, 11, 12)


def counts(pkg, log2n):
    """the block counts nsamp / H of the lane map: 1, 2, 5, and one below, at and one above one and two workgroup runs"""
    r = pkg.exc_run(log2n)
    return sorted({1, 2, 5, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1} - {0})


def random_window(N, seed):
    """a random legal window with 0 and 16384 in it: the first half anything in [0, 16384], the second what is left of 16384"""
    w = np.random.default_rng(seed).integers(0, 16385, N // 2, dtype=np.int64)
    w[0], w[N // 3], w[N // 2 - 1] = 0, 16384, 16384
    return np.concatenate([w, 16384 - w]).astype(np.int16)


def random_bins(N, share, seed):
    """bool [N]: about `share` of the bins, bin 0 and bin N - 1 among them where any"""
    b = np.random.default_rng(seed).random(N) < share
    if share > 0:
        b[0] = b[N - 1] = True
    return b


def median_thr(pkg, w, exc, hist=None):
    """the median cell power of w's segments under exc's window: about half of the cells lie above it"""
    L = int(exc.log2n)
    N, H = 1 << L, 1 << (L - 1)
    x = np.concatenate([np.zeros((N, 2), np.int64) if hist is None else np.asarray(hist, np.int64), np.asarray(w, np.int64)])
    sg = np.arange(min(w.shape[0] // H + 1, 8))
    X = pkg.psd_transform((x[sg[:, None] * H + np.arange(N)[None, :]] * exc.window()[None, :, None]) >> 1)
    return max(1, int(np.median((X * X).sum(-1))))


def on_device(pkg, synth, iq, exc, hist=None, noise=None, interf=None, nsamp=None, spare=0, guard=8):
    """the call on host array iq [n, 2] through device buffers -> (out int16 [nsamp, 2], hist_out, clipped, excised); the output
    buffer has `guard` sentinel samples behind it, which must come back untouched"""
    import torch
    n = iq.shape[0] - spare if nsamp is None else nsamp
    t = torch.from_numpy(np.ascontiguousarray(iq, np.int16)).cuda()
    o = torch.full((n + guard, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    hout, clipped, excised = synth.device_excise(t.data_ptr(), n, exc, o.data_ptr(), hist, noise, interf)
    out = o.cpu().numpy()
    assert (out[n:] == 0x5A5A).all(), "the sentinel behind d_out was written"
    return out[:n], hout, clipped, excised


def mirror(pkg, iq, exc, hist=None, noise=None, interf=None, nsamp=None):
    n = iq.shape[0] if nsamp is None else nsamp
    return pkg.excise_host(pkg.view_host(iq[:n], pkg.OUT_SC16, noise, interf=interf), exc, hist)


def compare(got, want, what=""):
    """findings (strings) of (out, hist_out, clipped, excised) against the same from the mirror"""
    bad = []
    for name, g, w in (("out", got[0], want[0]), ("hist_out", got[1], want[1])):
        if g.shape != w.shape or not (g == w).all():
            d = np.argwhere(g != w) if g.shape == w.shape else []
            bad.append("%s %s: %d components differ, first %s" % (what, name, len(d), "%s: %d, want %d" % (d[0].tolist(), g[tuple(d[0])], w[tuple(d[0])])
                                                                  if len(d) else "shape %r / %r" % (g.shape, w.shape)))
    for name, g, w in (("clipped", got[2], want[2]), ("excised", got[3], want[3])):
        if g != w:
            bad.append("%s %s: %d, want %d" % (what, name, g, w))
    return bad


def check(pkg, synth, iq, exc, hist=None, noise=None, interf=None, nsamp=None, what=""):
    return compare(on_device(pkg, synth, iq, exc, hist, noise, interf, nsamp), mirror(pkg, iq, exc, hist, noise, interf, nsamp), what)


def lane_map_plan(pkg, log2n, iq):
    """a random legal window, about 10 % of the bins masked, thr at the median cell power"""
    N = 1 << log2n
    e = pkg.Exc(log2n, 0, random_window(N, 0xE100 + log2n), random_bins(N, 0.1, 0xE200 + log2n))
    e.thr = median_thr(pkg, iq, e)
    return e


def lane_map(pkg, synth, log2n):
    """findings of every block count at one N, with and without a history, on one random buffer"""
    N, H = 1 << log2n, 1 << (log2n - 1)
    cs = counts(pkg, log2n)
    iq = ac.random_iq(cs[-1] * H, 0xE000 + log2n)
    e = lane_map_plan(pkg, log2n, iq)
    hist = ac.random_iq(N, 0xE300 + log2n)
    bad = []
    for nblk in cs:
        for h in (None, hist):
            bad += check(pkg, synth, iq, e, h, nsamp=nblk * H, what="N %d blocks %d hist %s" % (N, nblk, "none" if h is None else "random"))
    return bad


# ---- the inputs that press on the bound and on the clamp ----

def tone(amp, f, n):
    t = np.arange(n)
    return np.stack([np.rint(amp * np.cos(2 * np.pi * f * t)), np.rint(amp * np.sin(2 * np.pi * f * t))], 1).clip(-32768, 32767).astype(np.int16)


def stress_inputs(N, nblk=4):
    """name -> int16 [nblk * H, 2]: constant -32768, alternating full scale, full-scale tones on and between bins, +-full-scale
    random, an impulse"""
    n = nblk * (N // 2)
    rng = np.random.default_rng(0xE400 + N)
    alt = np.where((np.arange(n) & 1)[:, None] == 0, 32767, -32768) * np.ones((1, 2), np.int64)
    imp = np.zeros((n, 2), np.int16)
    imp[N // 2 + 3] = (32767, -32768)
    return {"constant -32768": np.full((n, 2), -32768, np.int16), "alternating": alt.astype(np.int16), "tone on a bin": tone(32767, 5.0 / N, n),
            "tone between bins": tone(32767, 5.5 / N, n), "random +-full scale": np.where(rng.random((n, 2)) < 0.5, -32768, 32767).astype(np.int16),
            "impulse": imp}


STRESS_SHARES = (0.0, 1.0 / 6, 1.0 / 2, 5.0 / 6)


def stress_plans(pkg, log2n):
    N = 1 << log2n
    base = pkg.exc_make(log2n)
    return [base.copy(bins=random_bins(N, sh, 0xE500 + log2n + int(60 * sh))) for sh in STRESS_SHARES]


def square_case(pkg, log2n):
    """a full-scale square wave of period N / 4 with every bin masked but 4 and N - 4: the fundamental alone is 4 / pi of full scale,
    the clamp works -> (iq, plan)"""
    N = 1 << log2n
    n = 4 * (N // 2)
    sq = np.where((np.arange(n) % (N // 4)) < N // 8, 32767, -32768)
    bins = np.ones(N, bool)
    bins[4] = bins[N - 4] = False
    return np.stack([sq, sq], 1).astype(np.int16), pkg.exc_make(log2n).copy(bins=bins)


def chirp_set(pkg, fs=FS):
    return fc.chirp_set(pkg, fs)


def advanced(pkg, noise, interf, n):
    return fc.advanced(pkg, noise, interf, n)


# ---- end to end: what excision is for ----

E2E_LOG2N, E2E_N, E2E_H = 8, 256, 128
E2E_NSAMP = 8192                           # 64 blocks; the search reads out[H : H + 7800], the cleaned w[0 : 7800]
E2E_NOISE = {"seed": 0xE2E, "sample0": (1 << 33) + 7, "sigma": 700.0, "shift": 1}
E2E_CW_HZ = 317e3
E2E_CW_JS_DB = 30.0                        # on the mirrors (e2e_cpu) the search loses PRNs from 10 dB on, all of them at 30 dB
E2E_CHIRP = (-1.25e6, 1.25e6, 0.79e-3)     # the README's full-band chirp: f0, f1, sweep time
E2E_CHIRP_JS_DB = 30.0                     # ... loses PRNs from 20 dB on, all of them at 30 dB
E2E_MASK_DB, E2E_THR_DB = 6.0, 9.0         # CW: the bins 6 dB above the median bin are masked; chirp: cells 9 dB above the quiet floor go


def e2e_descriptors(pkg):
    return ac.e2e_descriptors(pkg)


def cw_set(pkg, js_db=E2E_CW_JS_DB, fs=FS):
    return pkg.InterfSet([pkg.interf_make(pkg.INTERF_CW, js_db, E2E_CW_HZ, delt=1.0 / fs)], E2E_NOISE["shift"], E2E_NOISE["sample0"])


def sweep_set(pkg, js_db=E2E_CHIRP_JS_DB, fs=FS):
    f0, f1, t = E2E_CHIRP
    return pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, js_db, f0, f1, t, delt=1.0 / fs)], E2E_NOISE["shift"], E2E_NOISE["sample0"])


def e2e_plan(pkg, spectrum, nseg, psd_plan, kind):
    """the excision plan from a spectrum: for a CW emitter the mask, from the spectrum with the emitter in it; for a chirp, which
    fills every bin of an averaged spectrum and so lifts its median, the threshold, from the spectrum of the same buffer without
    the emitter (the floor a receiver has measured before the jammer came)"""
    base = pkg.exc_make(E2E_LOG2N)
    if kind == "cw":
        return pkg.exc_from_psd(base, spectrum, psd_plan, nseg, E2E_MASK_DB, 0.0)
    return pkg.exc_from_psd(base, spectrum, psd_plan, nseg, 0.0, E2E_THR_DB)


def e2e_psd_plan(pkg):
    return pkg.psd_make(E2E_LOG2N, E2E_NSAMP, 0, pkg.PSD_HANN)


def e2e_cpu(pkg):
    """the end-to-end cases on the CPU oracle's render with the mirrors alone -> findings; prints the figures"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_binding as ob
    bad = []
    ch = e2e_descriptors(pkg)
    iq = ob.Oracle().fill_blocks(ch, 1.0 / FS, E2E_NSAMP)[0][0]
    cfg = ac.e2e_cfg(pkg, pkg.OUT_SC16)
    pp = e2e_psd_plan(pkg)

    def wrong(w):
        rows, _ = pkg.acquire_host(w[:ac.E2E_NSAMP], cfg)
        f, present, absent = ac.e2e_findings(pkg, rows, cfg, ch)
        return f, min(present.values()), max(absent.values())

    f, lo, hi = wrong(pkg.view_host(iq, pkg.OUT_SC16, E2E_NOISE))
    print("noise alone: %d findings, present min %.2f, absent max %.2f" % (len(f), lo, hi))
    if f:
        bad.append("noise alone: " + "; ".join(f))
    for kind, js in (("cw", cw_set(pkg)), ("chirp", sweep_set(pkg))):
        w = pkg.view_host(iq, pkg.OUT_SC16, E2E_NOISE, interf=js)
        f0, lo0, hi0 = wrong(w)
        spectrum, nseg = pkg.psd_host(w if kind == "cw" else pkg.view_host(iq, pkg.OUT_SC16, E2E_NOISE), pp)
        e = e2e_plan(pkg, spectrum, nseg, pp, kind)
        out, _, clipped, excised = pkg.excise_host(w, e)
        f1, lo1, hi1 = wrong(out[E2E_H:])
        print("%s: before %d findings (present min %.2f, absent max %.2f); %d bins masked, thr %d, %d cells zeroed of %d, clipped %d; "
              "after %d findings (present min %.2f, absent max %.2f)" % (kind, len(f0), lo0, hi0, int(e.bins().sum()), int(e.thr), excised,
                                                                          E2E_NSAMP // E2E_H * E2E_N, clipped, len(f1), lo1, hi1))
        if not f0:
            bad.append("%s: the search is not defeated before excision" % kind)
        if f1:
            bad.append("%s after excision: %s" % (kind, "; ".join(f1)))
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
                print("N %d: blocks %s, with and without a history" % (1 << log2n, counts(pkg, log2n)), flush=True)
            iq = (ac.random_iq(40 * 128, 0xE5F).astype(np.int32) // 4).astype(np.int16)
            e = lane_map_plan(pkg, 8, iq)
            for what, nz, js in (("plain", None, None), ("noise", NOISE, None), ("noise + chirp", NOISE, chirp_set(pkg)), ("chirp", None, chirp_set(pkg))):
                bad += check(pkg, s, iq, e, None, nz, js, what=what)
            print("plain, noise, noise + chirp, chirp", flush=True)
    if bad:
        print("\n".join(bad))
        return 1
    print("the excision is bit-exact against the numpy mirror" if not cpu else "the end-to-end figures hold on the mirror")
    return 0


if __name__ == "__main__":
    sys.exit(main())
