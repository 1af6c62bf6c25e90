"""Would a cold receiver find these satellites?  RINEX file -> front end -> one batch on the GPU -> gpsbb_device_acquire on the
first block in the view of each output format (SC16, SC8 at a shift, SC1), optionally with the library's noise (-W) and one
emitter (-J) -> per PRN the bin, delay and ratio found, beside what the descriptors say.

    python tools/acq_report.py [-e tests/golden/synth3540.14n] [-W cn0[,shift]] [-J chirp,f0_hz,f1_hz,sweep_s | cw,f_hz] [-L js_db]
                               [-q sc8_shift] [-s fs] [-c coh_s] [-n nnc] [-b f_min,f_step,nbins] [-o OUT]

-W and -J as tools/jam_report.py takes them (default: neither).  A PRN counts as found where its ratio (peak over the PRN's mean
cell) is above twice the largest ratio among the PRNs that are not in the block.  Default output: profiles/aq01_acq_report.txt.
"""
import argparse
import math
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)
except Exception:
    pass
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-e", default=os.path.join(ROOT, "tests", "golden", "synth3540.14n"))
    ap.add_argument("-W", default="")
    ap.add_argument("-J", default="")
    ap.add_argument("-L", type=float, default=20.0)
    ap.add_argument("-q", type=int, default=-1)
    ap.add_argument("-s", type=float, default=2.6e6)
    ap.add_argument("-c", type=float, default=1e-3)
    ap.add_argument("-n", type=int, default=2)
    ap.add_argument("-b", default="-5000,500,21")
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "aq01_acq_report.txt"))
    a = ap.parse_args()
    fs, delt = a.s, 1.0 / a.s
    f_min, f_step, nbins = float(a.b.split(",")[0]), float(a.b.split(",")[1]), int(a.b.split(",")[2])
    nz = js = None
    nshift = 0
    sigma = 0.0
    if a.W:
        cn0 = float(a.W.split(",")[0])
        nshift = int(a.W.split(",")[1]) if "," in a.W else 0
        sigma = pkg.noise_sigma(cn0, 1.0, delt)
        nz = pkg.Noise(1, 0, sigma, nshift, 0)
    if a.J:
        spec = a.J.split(",")
        e = (pkg.interf_make(pkg.INTERF_CW, a.L, float(spec[1]), delt=delt) if spec[0] == "cw" else
             pkg.interf_make(pkg.INTERF_CHIRP, a.L, float(spec[1]), float(spec[2]), float(spec[3]), delt=delt))
        js = pkg.InterfSet([e], nshift, 0)
    level = max(sigma, 150.0) / (1 << nshift)
    shift8 = a.q if a.q >= 0 else max(0, math.ceil(math.log2(level / 32.0)))
    views = (("sc16", pkg.OUT_SC16), ("sc8>>%d" % shift8, pkg.OUT_SC8(shift8)), ("sc1", pkg.OUT_SC1))
    cfgs = {name: pkg.acq_make(delt, f_min, f_step, nbins, a.c, 0, a.n, fmt) for name, fmt in views}
    c0 = cfgs["sc16"]
    nsamp = c0.nnc * c0.ncoh + c0.nlags - 1
    pkg.build_frontend()
    fe = pkg.FrontEnd(a.e, llh=(30.286502, 120.032669, 100.0), max_chan=12)
    ch = fe.generate(1)
    fe.close()
    rows = {}
    with pkg.Synth(0) as s:
        b = s.batch(ch, delt, nsamp)
        b.run()
        s.sync()
        for name, fmt in views:
            rows[name] = s.device_acquire(b.device_iq(), nsamp, cfgs[name], fmt, nz, js)
        b.close()
    present = {int(d["prn"]): d for d in ch[0] if d["prn"] > 0}
    lines = ["# %s, %.4g MS/s, one block of %d samples; %d bins from %g Hz in steps of %g Hz, %d x %d samples coherent, %d delays"
             % (os.path.basename(a.e), fs / 1e6, nsamp, nbins, f_min, f_step, c0.nnc, c0.ncoh, c0.nlags),
             "# noise: %s; emitter: %s" % ("%s dB-Hz for a gain-1.0 channel (sigma %.1f, shift %d)" % (a.W.split(",")[0], sigma, nshift) if a.W else "none",
                                          "%s at J/S %+.0f dB" % (a.J, a.L) if a.J else "none"),
             "# view      PRN   gain  f_carr   bin(Hz) found   delay  found    ratio  (found: above twice the largest absent ratio)"]
    for name, _ in views:
        cfg = cfgs[name]
        best = {prn: pkg.acq_best(rows[name], cfg, prn) for prn in range(1, 33)}
        floor = max(r[3] for prn, r in best.items() if prn not in present)
        nfound = 0
        for prn, d in sorted(present.items()):
            k, lag, _, ratio = best[prn]
            want_lag = ((1023.0 - float(d["code_phase"])) / (float(d["f_code"]) * delt)) % cfg.nlags
            off = abs(lag - want_lag)
            ok = ratio > 2.0 * floor and min(off, cfg.nlags - off) <= 1.0 and abs(f_min + k * f_step - float(d["f_carr"])) <= abs(f_step)
            nfound += ok
            lines.append("%-9s %4d %6.3f %7.0f %9.0f %5s %7.1f %6d %8.1f" % (name, prn, float(d["gain"]), float(d["f_carr"]), f_min + k * f_step,
                                                                               "yes" if ok else "no", want_lag, lag, ratio))
        lines.append("%-9s found %d of %d; largest absent ratio %.1f" % (name, nfound, len(present), floor))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
