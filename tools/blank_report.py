"""What blanking buys a receiver under a pulsed emitter: RINEX file -> front end -> one batch of 8192 samples on the GPU, under the
library's noise (-W) and a pulsed CW emitter (-J f_hz,period_s,duty at -L dB J/S) -> per PRN whether the search finds its cell and
the C/N0 its peak implies: without the emitter, with it, after gpsbb_device_blank (the plan from gpsbb_device_level over blocks of
64 samples and gpsbb_blank_from_level, L = G = hold = 8) and, for comparison, after gpsbb_device_excise at N = 256 with a
threshold -t dB above the median of the spectrum without the emitter — the notch's best answer to a pulse: it zeroes the cells of
the segments the pulse touches.  That comparison is what the tool is for; it prints and promises nothing.

The C/N0 is read off the search's own figure as tools/exc_report.py reads it: with a coherent time T the peak implies
C/N0 = 10 log10(max(ratio - 1, 0) / T) dB-Hz; below about 36 dB-Hz it is the floor's own largest cell that speaks.  A PRN counts as
found where its ratio is above twice the largest ratio among the PRNs that are not in the block and its cell is the descriptors'.
Every blanked output is compared == with the numpy mirror on the way.

    python tools/blank_report.py [-e tests/golden/synth3540.14n] [-W cn0[,shift]] [-J f_hz,period_s,duty] [-L js_db] [-d thr_db] [-t exc_thr_db]
                                 [-o profiles/bl01_blank_report.txt]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (one HIP runtime for torch and libgpsbb)

from __graft_entry__ import load_package  # noqa: E402
import blank_check as bc  # noqa: E402

T_COH = 1e-3
FS = bc.FS
NSAMP, SEARCH = 8192, 7800
SHAPE, BLOCK, EXC_LOG2N = (8, 8, 8), 64, 8


def cn0(ratio):
    return 10.0 * math.log10(max(ratio - 1.0, 1e-9) / T_COH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-e", default=os.path.join(ROOT, "tests", "golden", "synth3540.14n"))
    ap.add_argument("-W", default="47,1")
    ap.add_argument("-J", default="317e3,0.7e-3,0.10")
    ap.add_argument("-L", type=float, default=40.0)
    ap.add_argument("-d", type=float, default=6.0)
    ap.add_argument("-t", type=float, default=9.0)
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "bl01_blank_report.txt"))
    a = ap.parse_args()
    pkg = load_package()
    delt = 1.0 / FS
    cn0_w = float(a.W.split(",")[0])
    nshift = int(a.W.split(",")[1]) if "," in a.W else 0
    nz = pkg.Noise(1, 0, pkg.noise_sigma(cn0_w, 1.0, delt), nshift, 0)
    f_hz, period_s, duty = (float(v) for v in a.J.split(","))
    js = pkg.InterfSet([pkg.interf_make(pkg.INTERF_CW, a.L, f_hz, pulse_period_s=period_s, duty=duty, delt=delt)], nshift, 0)
    pkg.build_frontend()
    fe = pkg.FrontEnd(a.e, llh=(30.286502, 120.032669, 100.0), max_chan=12)
    ch = fe.generate(1)
    fe.close()
    present = {int(d["prn"]): d for d in ch[0] if d["prn"] > 0}
    cfg = pkg.acq_make(delt, -5000.0, 500.0, 21, T_COH, 0, 2, pkg.OUT_SC16)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def per_prn(rows):
        best = {prn: pkg.acq_best(rows, cfg, prn) for prn in range(1, 33)}
        floor = max(r[3] for prn, r in best.items() if prn not in present)
        out = {}
        for prn, d in sorted(present.items()):
            k, lag, _, ratio = best[prn]
            want = ((1023.0 - float(d["code_phase"])) / (float(d["f_code"]) * delt)) % cfg.nlags
            off = abs(lag - want)
            ok = ratio > 2.0 * floor and min(off, cfg.nlags - off) <= 1.0 and abs(-5000.0 + 500.0 * k - float(d["f_carr"])) <= 500.0
            out[prn] = (ok, cn0(ratio))
        return out

    def row(what, r):
        say("%-26s" % what + "  ".join("%2d %5.1f%s" % (p, c, "*" if ok else " ") for p, (ok, c) in r.items()) + "   found %d of %d" % (
            sum(ok for ok, _ in r.values()), len(r)))

    with pkg.Synth(0) as s:
        b = s.batch(ch, delt, NSAMP)
        b.run()
        s.sync()
        iq, d_iq = b.read()[0][0], b.device_iq()
        say("# %s, %.4g MS/s, %d samples; noise %g dB-Hz for a gain-1.0 channel at shift %d; a CW emitter at %g Hz pulsed with period %g s and "
            "duty %g at J/S %g dB" % (os.path.basename(a.e), FS / 1e6, NSAMP, cn0_w, nshift, f_hz, period_s, duty, a.L))
        say("# per PRN the C/N0 in dB-Hz its peak implies, * where the search finds the PRN's cell")
        row("no emitter:", per_prn(s.device_acquire(d_iq, SEARCH, cfg, pkg.OUT_SC16, nz)))
        row("pulsed emitter:", per_prn(s.device_acquire(d_iq, SEARCH, cfg, pkg.OUT_SC16, nz, js)))
        out = torch.zeros((NSAMP, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        plan = pkg.blank_from_level(pkg.Blank(*SHAPE), s.device_level(d_iq, NSAMP // BLOCK, BLOCK, nz, js), nshift, a.d)
        hist, blanked, triggers = s.device_blank(d_iq, NSAMP, plan, out.data_ptr(), None, nz, js)
        bad = bc.compare((out.cpu().numpy(), hist, blanked, triggers), bc.mirror(pkg, iq, plan, None, nz, js))
        row("... blanked:", per_prn(s.device_acquire(out.data_ptr() + 4 * SHAPE[1], SEARCH, cfg)))
        say("#   thr %d (%g dB above the median block), %d triggers, %d of %d samples blanked (%.1f %%)%s" % (
            int(plan.thr), a.d, triggers, blanked, NSAMP, 100.0 * blanked / NSAMP, "" if not bad else "; NOT the mirror: " + "; ".join(bad)))
        pp = pkg.psd_make(EXC_LOG2N, NSAMP, 0, pkg.PSD_HANN)
        spectrum, nseg = s.device_psd(d_iq, NSAMP, pp, pkg.OUT_SC16, nz)
        e = pkg.exc_from_psd(pkg.exc_make(EXC_LOG2N), spectrum, pp, nseg, 0.0, a.t)
        _, clipped, excised = s.device_excise(d_iq, NSAMP, e, out.data_ptr(), None, nz, js)
        H = 1 << (EXC_LOG2N - 1)
        row("... excised instead:", per_prn(s.device_acquire(out.data_ptr() + 4 * H, SEARCH, cfg)))
        say("#   N %d, thr %d (%g dB above the quiet spectrum's median), %.1f %% of the cells zeroed, %d clipped" % (
            1 << EXC_LOG2N, int(e.thr), a.t, 100.0 * excised / (NSAMP // H * (1 << EXC_LOG2N)), clipped))
        b.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
