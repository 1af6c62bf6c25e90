"""gpsbb_device_acquire against the numpy restatement (acquire_host over view_host): the cases and the comparison that
tests/test_acquire.py and tests/test_acquire_gpu.py share.  Every comparison is == on integers.  Run as a script it checks the
cases on the GPU and prints what it compared:

    python tools/acq_check.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FS = 2.6e6
STEPS3 = (0, 0x01234567, -0x0089ABCD)
NOISE = {"seed": 0xACC01, "sample0": (1 << 32) + 54321, "sigma": 700.0, "shift": 1}   # sample0 above 2^32 and odd


def code_step(fs=FS):
    """nearbyint(ldexp(1.023e6 / fs, 32)), as gpsbb_acq_make has it"""
    return int(np.rint(math.ldexp(1.023e6 * (1.0 / fs), 32)))


def make_cfg(pkg, steps, ncoh, nlags, nnc, view, prn_mask=0xFFFFFFFF, shift=None, fs=FS):
    """a configuration from its integers; shift None: the smallest legal one"""
    c = pkg.AcqCfg()
    c.prn_mask, c.nbins, c.code_step, c.ncoh, c.nlags, c.nnc = prn_mask, len(steps), code_step(fs), ncoh, nlags, nnc
    for k, s in enumerate(steps):
        c.step[k] = s
    c.shift = pkg.acq_min_shift(view, ncoh, nnc) if shift is None else shift
    return c


def mask_of(prns):
    return sum(1 << (p - 1) for p in prns)


def random_iq(nsamp, seed):
    """random int16 pairs over the whole range, the three extremes among them, in both components"""
    rng = np.random.default_rng(seed)
    iq = rng.integers(-32768, 32768, size=(nsamp, 2), dtype=np.int64).astype(np.int16)
    ext = np.array([32767, -32767, -32768], np.int16)
    iq[1:4, 0] = ext
    iq[2:5, 1] = ext
    iq[nsamp - 1] = (-32768, 32767)
    return iq


def compare(got_rows, got_grid, want_rows, want_grid, what=""):
    """findings (strings): rows field by field and, where given, the whole grid"""
    bad = []
    for f in ("peak", "lag", "sum_lo", "sum_hi", "_pad"):
        if got_rows.shape != want_rows.shape or not (got_rows[f] == want_rows[f]).all():
            w = np.argwhere(got_rows[f] != want_rows[f]) if got_rows.shape == want_rows.shape else []
            bad.append("%s rows.%s: %d differ, first (prn - 1, bin) %s" % (what, f, len(w), w[0].tolist() if len(w) else "shape"))
    if got_grid is not None:
        if got_grid.shape != want_grid.shape or not (got_grid == want_grid).all():
            w = np.argwhere(got_grid != want_grid) if got_grid.shape == want_grid.shape else []
            bad.append("%s grid: %d cells differ, first (prn - 1, bin, delay) %s" % (what, len(w), w[0].tolist() if len(w) else "shape"))
    return bad


def on_device(pkg, synth, iq, cfg, view=0, noise=None, interf=None, nsamp=None):
    """the search of host array iq [n, 2] through a device buffer -> (rows, grid)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(iq, np.int16)).cuda()
    torch.cuda.synchronize()
    return synth.device_acquire(t.data_ptr(), iq.shape[0] if nsamp is None else nsamp, cfg, view, noise, interf, want_grid=True)


def check(pkg, synth, iq, cfg, view=0, noise=None, interf=None, nsamp=None, what=""):
    """findings of one call against the mirror fed with view_host's output of the first nsamp samples"""
    n = iq.shape[0] if nsamp is None else nsamp
    got = on_device(pkg, synth, iq, cfg, view, noise, interf, nsamp)
    want = pkg.acquire_host(pkg.view_host(iq[:n], view, noise, interf=interf), cfg)
    return compare(got[0], got[1], want[0], want[1], what)


def lane_map_case(pkg):
    """all 32 PRNs, N = 96 (three K-steps), P = 40 (a whole delay tile and a ragged one), three bins, one interval"""
    cfg = make_cfg(pkg, STEPS3, 96, 40, 1, pkg.OUT_SC16)
    return random_iq(96 + 40 - 1, 0xA1), cfg


def ragged_case(pkg, view=0, spare=0):
    """N = 1000 (a ragged K-step, four staged chunks), P = 70 (three tiles), 3 intervals, PRNs {1, 17, 32}, 2 bins; nsamp exactly
    nnc * N + P - 1, plus `spare` samples of 0x7fff behind them"""
    cfg = make_cfg(pkg, (0x00345678, -0x01abcdef), 1000, 70, 3, view, prn_mask=mask_of((1, 17, 32)))
    n = 3 * 1000 + 70 - 1
    iq = random_iq(n, 0xA2)
    if spare:
        iq = np.concatenate([iq, np.full((spare, 2), 0x7FFF, np.int16)])
    return iq, cfg, n


# ---- end to end: six satellites rendered, found by a search that is told nothing ----

E2E_NSAMP = 7800
E2E_PRESENT = (1, 2, 3, 4, 5, 6)


def e2e_descriptors(pkg):
    return pkg.synth_descriptors(1, nch=6, seed=0xACC)


def e2e_cfg(pkg, view):
    return pkg.acq_make(1.0 / FS, -5000.0, 500.0, 21, 1e-3, 0, 2, view)


def e2e_findings(pkg, rows, cfg, ch):
    """(findings, present ratios, absent ratios): per present PRN the bin nearest f_carr and a delay within 1 sample, circularly in
    P, of ((1023 - code_phase) / (f_code * delt)) mod P; every present ratio above twice the largest absent one"""
    delt = 1.0 / FS
    P = int(cfg.nlags)
    bad, present, absent = [], {}, {}
    for prn in range(1, 33):
        b, lag, _, ratio = pkg.acq_best(rows, cfg, prn)
        if prn not in E2E_PRESENT:
            absent[prn] = ratio
            continue
        present[prn] = ratio
        d = ch[0, prn - 1]
        assert int(d["prn"]) == prn
        want_bin = int(np.argmin([abs(-5000.0 + 500.0 * k - float(d["f_carr"])) for k in range(21)]))
        want_lag = ((1023.0 - float(d["code_phase"])) / (float(d["f_code"]) * delt)) % P
        off = abs(lag - want_lag)
        off = min(off, P - off)
        if b != want_bin or off > 1.0:
            bad.append("PRN %d: bin %d (want %d), delay %d (want %.2f)" % (prn, b, want_bin, lag, want_lag))
    if min(present.values()) <= 2.0 * max(absent.values()):
        bad.append("ratios: present min %.2f, absent max %.2f" % (min(present.values()), max(absent.values())))
    return bad, present, absent


def main():
    sys.path.insert(0, ROOT)
    try:
        import torch  # noqa: F401  (one HIP runtime for torch and libgpsbb)
    except Exception:
        pass
    from __graft_entry__ import load_package
    pkg = load_package()
    bad = []
    with pkg.Synth(0) as s:
        iq, cfg = lane_map_case(pkg)
        bad += check(pkg, s, iq, cfg, what="lane map")
        print("lane map: 32 PRNs x 3 bins x 40 delays", flush=True)
        for view in (pkg.OUT_SC16, pkg.OUT_SC8(5), pkg.OUT_SC1):
            iq, cfg, n = ragged_case(pkg, view)
            bad += check(pkg, s, iq, cfg, view, what="ragged 0x%x" % view)
            bad += check(pkg, s, iq, cfg, view, NOISE, what="ragged 0x%x noise" % view)
            print("ragged, view 0x%x: plain and with noise" % view, flush=True)
    if bad:
        print("\n".join(bad))
        return 1
    print("acquisition bit-exact against the numpy mirror")
    return 0


if __name__ == "__main__":
    sys.exit(main())
