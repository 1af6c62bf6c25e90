"""gpsbb_device_blank against the numpy restatement (blank_host over view_host): the cases and the comparison that
tests/test_blank.py and tests/test_blank_gpu.py share.  Every comparison is == on integers: every output sample, the history
handed on and both counters.  Run as a script it checks the cases on the GPU and prints what it compared; --cpu runs the
end-to-end case (six satellites under noise and a pulsed CW emitter, acquired before and after blanking) with the CPU oracle's
render and the numpy mirrors only, and prints the figures the GPU test asserts:

    python tools/blank_check.py [--cpu]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402
import exc_check as ec  # noqa: E402
import fir_check as fc  # noqa: E402

FS = ac.FS
NOISE = ac.NOISE
SHAPES = ((1, 0, 0), (8, 8, 8), (64, 255, 1023), (64, 0, 0), (1, 255, 0), (1, 0, 1023))   # (L, G, hold): both ends of every range
FULL = (-32768, -32768)                    # the sample of the largest power, 2^31


def plan(pkg, shape, thr):
    L, G, hold = shape
    return pkg.Blank(L, G, hold, thr)


def random_thr(shape, iq):
    """a threshold that the buffer iq passes now and then: the boxcar sums of iq behind zeros, the k-th largest of them less one,
    k at least 3, at most 4 % of the samples and about two per dilated length, so that triggers come in a few groups and some of
    the output survives them"""
    L, G, hold = shape
    p = (np.asarray(iq, np.int64) ** 2).sum(1)
    cp = np.concatenate([np.zeros(L, np.int64), np.cumsum(p)])
    s = np.sort(cp[L:] - cp[:-L])
    k = min(max(3, int(s.size * min(0.04, 2.0 / (G + hold + L)))), s.size)
    return max(int(s[s.size - k]) - 1, 0)


def lengths(pkg, K):
    """the sample counts of the tile map: 1, 2, around the history's length, around one and two tiles and around a workgroup's run"""
    Tt, r = pkg.BLANK_TILE, pkg.BLANK_MIN_RUN
    return sorted({1, 2, K, K + 1, Tt - 1, Tt, Tt + 1, 2 * Tt + 1, r * Tt - 1, r * Tt, r * Tt + 1} - {0})


def on_device(pkg, synth, iq, blank, hist=None, noise=None, interf=None, nsamp=None, spare=0, guard=8):
    """the call on host array iq [n, 2] through device buffers -> (out int16 [nsamp, 2], hist_out, blanked, triggers); the output
    buffer has `guard` sentinel samples behind it, which must come back untouched"""
    import torch
    n = iq.shape[0] - spare if nsamp is None else nsamp
    t = torch.from_numpy(np.ascontiguousarray(iq, np.int16)).cuda()
    o = torch.full((n + guard, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    hout, blanked, triggers = synth.device_blank(t.data_ptr(), n, blank, o.data_ptr(), hist, noise, interf)
    out = o.cpu().numpy()
    assert (out[n:] == 0x5A5A).all(), "the sentinel behind d_out was written"
    return out[:n], hout, blanked, triggers


def mirror(pkg, iq, blank, hist=None, noise=None, interf=None, nsamp=None):
    n = iq.shape[0] if nsamp is None else nsamp
    return pkg.blank_host(pkg.view_host(iq[:n], pkg.OUT_SC16, noise, interf=interf), blank, hist)


def compare(got, want, what=""):
    """findings (strings) of (out, hist_out, blanked, triggers) against the same from the mirror"""
    bad = []
    for name, g, w in (("out", got[0], want[0]), ("hist_out", got[1], want[1])):
        if g.shape != w.shape or not (g == w).all():
            d = np.argwhere(g != w) if g.shape == w.shape else []
            bad.append("%s %s: %d components differ, first %s" % (what, name, len(d), "%s: %d, want %d" % (d[0].tolist(), g[tuple(d[0])], w[tuple(d[0])])
                                                                  if len(d) else "shape %r / %r" % (g.shape, w.shape)))
    for name, g, w in (("blanked", got[2], want[2]), ("triggers", got[3], want[3])):
        if g != w:
            bad.append("%s %s: %d, want %d" % (what, name, g, w))
    return bad


def check(pkg, synth, iq, blank, hist=None, noise=None, interf=None, nsamp=None, what=""):
    return compare(on_device(pkg, synth, iq, blank, hist, noise, interf, nsamp), mirror(pkg, iq, blank, hist, noise, interf, nsamp), what)


def random_hist(K, seed):
    return ac.random_iq(max(K, 5), seed)[:K]


def tile_map(pkg, synth, shape):
    """findings of every sample count of one (L, G, hold), with and without a history, on one random buffer"""
    K = sum(shape) - 1
    ns = lengths(pkg, K)
    iq = ac.random_iq(ns[-1], 0xB100 + K)
    b = plan(pkg, shape, random_thr(shape, iq))
    hist = random_hist(K, 0xB200 + K)
    bad = []
    for n in ns:
        for h in (None, hist):
            bad += check(pkg, synth, iq, b, h, nsamp=n, what="(L, G, hold) %r nsamp %d hist %s" % (shape, n, "none" if h is None else "random"))
    return bad


def planted(n, at, seed, sigma=20.0):
    """a quiet Gaussian background of n samples with single full-scale samples at the positions `at`"""
    iq = np.clip(np.rint(np.random.default_rng(seed).standard_normal((n, 2)) * sigma), -32768, 32767).astype(np.int16)
    for j in at:
        iq[j] = FULL
    return iq


def blanked_by(n, K, G, hits):
    """bool [n]: the outputs a full-scale sample at each input position of `hits` (negative: inside the history) zeroes on a
    background that triggers nothing: it sits in the boxcar of trig[j] .. trig[j + L - 1], which blank j - G .. j + L - 1 + hold of the
    input and so the outputs j .. j + G + hold + L - 1 = j + K"""
    z = np.zeros(n, bool)
    for j in hits:
        z[max(j, 0):max(min(j + K + 1, n), 0)] = True
    return z


# ---- end to end: what blanking is for ----

E2E_NSAMP = ec.E2E_NSAMP                   # 8192; the search reads out[G : G + 7800], the blanked w[0 : 7800]
E2E_NOISE = ec.E2E_NOISE
E2E_CW_HZ = ec.E2E_CW_HZ
E2E_JS_DB = 40.0                           # nothing saturates int16 up to 40 dB
E2E_PERIOD_S, E2E_DUTY = 0.7e-3, 0.10      # 1820 samples, 182 of them on
E2E_SHAPE = (8, 8, 8)                      # L = G = hold = 8
E2E_BLOCK = 64                             # the levels' blocks: short against the pulse period, 128 of them
E2E_THR_DB = 6.0                           # above the lower median of the blocks' levels; the issue's value held every assertion
E2E_MAX_BLANKED = 0.12                     # the duty plus (G + hold + L) / 1820 per pulse, rounded up
E2E_MAX_QUIET = 0.001                      # of the buffer without the emitter under the same plan


def pulsed_set(pkg, js_db=E2E_JS_DB, fs=FS):
    return pkg.InterfSet([pkg.interf_make(pkg.INTERF_CW, js_db, E2E_CW_HZ, pulse_period_s=E2E_PERIOD_S, duty=E2E_DUTY, delt=1.0 / fs)],
                         E2E_NOISE["shift"], E2E_NOISE["sample0"])


def e2e_plan(pkg, levels, thr_db=E2E_THR_DB):
    """the plan from the levels of the jammed buffer's blocks of E2E_BLOCK samples (device_level's or level_host's)"""
    return pkg.blank_from_level(plan(pkg, E2E_SHAPE, 0), levels, E2E_NOISE["shift"], thr_db)


def e2e_budget(blanked, quiet, n=E2E_NSAMP):
    """findings of the two shares the end-to-end case bounds"""
    bad = []
    if blanked > E2E_MAX_BLANKED * n:
        bad.append("blanked %d of %d: more than %.0f %%" % (blanked, n, 100 * E2E_MAX_BLANKED))
    if quiet > E2E_MAX_QUIET * n:
        bad.append("the quiet buffer: blanked %d of %d: more than %.1f %%" % (quiet, n, 100 * E2E_MAX_QUIET))
    return bad


def e2e_cpu(pkg):
    """the end-to-end case on the CPU oracle's render with the mirrors alone -> findings; prints the figures"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_binding as ob
    bad = []
    ch = ec.e2e_descriptors(pkg)
    n, G = E2E_NSAMP, E2E_SHAPE[1]
    iq = ob.Oracle().fill_blocks(ch, 1.0 / FS, n)[0][0]
    cfg = ac.e2e_cfg(pkg, pkg.OUT_SC16)

    def wrong(w):
        rows, _ = pkg.acquire_host(w[:ac.E2E_NSAMP], cfg)
        f, present, absent = ac.e2e_findings(pkg, rows, cfg, ch)
        return f, min(present.values()), max(absent.values())

    quiet = pkg.view_host(iq, pkg.OUT_SC16, E2E_NOISE)
    f, lo, hi = wrong(quiet)
    print("noise alone: %d findings, present min %.2f, absent max %.2f" % (len(f), lo, hi))
    if f:
        bad.append("noise alone: " + "; ".join(f))
    js = pulsed_set(pkg)
    w = pkg.view_host(iq, pkg.OUT_SC16, E2E_NOISE, interf=js)
    f0, lo0, hi0 = wrong(w)
    b = e2e_plan(pkg, pkg.level_host(iq.reshape(n // E2E_BLOCK, E2E_BLOCK, 2), E2E_NOISE, js))
    out, _, blanked, triggers = pkg.blank_host(w, b)
    f1, lo1, hi1 = wrong(out[G:])
    _, _, quiet_blanked, _ = pkg.blank_host(quiet, b)
    print("pulsed emitter: before %d findings (present min %.2f, absent max %.2f); thr %d, %d triggers, %d of %d blanked (%.1f %%), "
          "%d of the quiet buffer; after %d findings (present min %.2f, absent max %.2f)" % (
              len(f0), lo0, hi0, int(b.thr), triggers, blanked, n, 100.0 * blanked / n, quiet_blanked, len(f1), lo1, hi1))
    if not f0:
        bad.append("the search is not defeated before blanking")
    if f1:
        bad.append("after blanking: %s" % "; ".join(f1))
    return bad + e2e_budget(blanked, quiet_blanked)


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
            for shape in SHAPES:
                bad += tile_map(pkg, s, shape)
                print("(L, G, hold) %r: nsamp %s, with and without a history" % (shape, lengths(pkg, sum(shape) - 1)), flush=True)
            iq = (ac.random_iq(2 * pkg.BLANK_TILE + 77, 0xB5F).astype(np.int32) // 4).astype(np.int16)
            b = plan(pkg, (8, 8, 8), random_thr((8, 8, 8), pkg.view_host(iq, pkg.OUT_SC16, NOISE)))
            for what, nz, js in (("plain", None, None), ("noise", NOISE, None), ("noise + chirp", NOISE, fc.chirp_set(pkg)), ("chirp", None, fc.chirp_set(pkg))):
                bad += check(pkg, s, iq, b, None, nz, js, what=what)
            print("plain, noise, noise + chirp, chirp", flush=True)
    if bad:
        print("\n".join(bad))
        return 1
    print("the blanker is bit-exact against the numpy mirror" if not cpu else "the end-to-end figures hold on the mirror")
    return 0


if __name__ == "__main__":
    sys.exit(main())
