"""Does a receiver hold these satellites, and does it read their data bits?  RINEX file -> front end -> a chained batch on the GPU
(one buffer of consecutive blocks) -> gpsbb_device_acquire on its first 3 ms -> gpsbb_trk_seed per satellite found ->
gpsbb_device_track over the whole buffer, in the view of each output format (SC16, SC8 at a shift, SC1), optionally with the
library's noise (-W) and one emitter (-J) -> per PRN: the carrier the loop settled on beside the last block's f_carr, where the
data bits turn beside the descriptor's icode, and how many of the bits read back agree with the front end's (up to the Costas
loop's one sign per channel).

    python tools/track_report.py [-e tests/golden/synth3540.14n] [-W cn0[,shift]] [-J chirp,f0_hz,f1_hz,sweep_s | cw,f_hz] [-L js_db]
                                 [-q sc8_shift] [-s fs] [-d seconds] [-k skip] [-o OUT]

-W and -J as tools/acq_report.py takes them (default: neither).  "lock": one bit edge carries more than half of the sign changes
and every bit agrees.  Default output: profiles/tk01_track_report.txt.
"""
import argparse
import math
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import torch  # noqa: F401  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)
except Exception:
    pass
import numpy as np  # noqa: E402

import track_check as tc  # noqa: E402
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
    ap.add_argument("-d", type=float, default=0.5)
    ap.add_argument("-k", type=int, default=150)
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "tk01_track_report.txt"))
    a = ap.parse_args()
    fs, delt = a.s, 1.0 / a.s
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
    nsamp = int(round(fs * 0.1))   # the front end's blocks are 0.1 s (the reference's)
    nblocks = max(2, int(round(a.d * 10)))
    total = nblocks * nsamp
    pkg.build_frontend()
    fe = pkg.FrontEnd(a.e, llh=(30.286502, 120.032669, 100.0), max_chan=12)
    ch = fe.generate(nblocks)
    fe.close()
    present = {int(d["prn"]): k for k, d in enumerate(ch[0]) if d["prn"] > 0 and (ch["prn"][:, k] == d["prn"]).all()}
    trk = pkg.trk_make(delt, max_epochs=int(total * 1.023e6 * delt / 1023) + 8)
    out = {}
    with pkg.Synth(0) as s:
        b = s.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
        b.run()
        s.sync()
        for name, fmt in views:
            acq = pkg.acq_make(delt, -5000.0, 250.0, 41, 1e-3, 0, 2, fmt)
            rows = s.device_acquire(b.device_iq(), acq.nnc * acq.ncoh + acq.nlags - 1, acq, fmt, nz, js)
            prns = sorted(present)
            st = np.zeros(len(prns), pkg.TRK_STATE_DTYPE)
            for k, prn in enumerate(prns):
                kb, lag, _, _ = pkg.acq_best(rows, acq, prn)
                st[k] = pkg.trk_seed(acq, prn, kb, lag)
            out[name] = (prns, s.device_track(b.device_iq(), total, trk, st, fmt, nz, js)[1])
        b.close()
    lines = ["# %s, %.4g MS/s, %d chained blocks of %d samples (%.1f s) as one buffer; seeded by a search of 41 bins of 250 Hz over 2 x 1 ms"
             % (os.path.basename(a.e), fs / 1e6, nblocks, nsamp, nblocks * 0.1),
             "# loops: kf %d, kp1 %d, kp2 %d, kd1 %d, %d epochs of FLL; bit edge and bits from record %d on" % (trk.kf, trk.kp1, trk.kp2, trk.kd1, trk.nfll, a.k),
             "# noise: %s; emitter: %s" % ("%s dB-Hz for a gain-1.0 channel (sigma %.1f, shift %d)" % (a.W.split(",")[0], sigma, nshift) if a.W else "none",
                                          "%s at J/S %+.0f dB" % (a.J, a.L) if a.J else "none"),
             "# view      PRN   gain    f_carr   tracked    edge want   bits agree  min|P.i|  max|P.q|  lock"]
    for name, _ in views:
        prns, recs = out[name]
        nlock = 0
        for prn, r in zip(prns, recs):
            d0, d1 = ch[0, present[prn]], ch[-1, present[prn]]
            if r.size < a.k + 40:
                lines.append("%-9s %4d: %d records" % (name, prn, r.size))
                continue
            f = float(np.mean(r["carr_step"][-50:].astype(np.float64))) / float(1 << 48) * fs
            off, hist = pkg.trk_bitsync(r, a.k)
            first = a.k + ((off - a.k) % 20)
            bits = pkg.trk_bits(r, first)
            want = tc.want_bits(d0, first, bits.size)
            agree = max(int((bits == want).sum()), int((bits == -want).sum()))
            want_off = (-(int(d0["icode"]) + 1)) % 20
            ok = agree == bits.size and off == want_off and 2 * int(hist[off]) > int(hist.sum())
            nlock += ok
            lines.append("%-9s %4d %6.3f %9.1f %9.1f %7d %4d %6d %5d %9.3g %9.3g  %s"
                         % (name, prn, float(d0["gain"]), float(d1["f_carr"]), f, off, want_off, bits.size, agree,
                            float(np.abs(r["p_i"][a.k:]).min()), float(np.abs(r["p_q"][a.k:]).max()), "yes" if ok else "no"))
        lines.append("%-9s lock on %d of %d" % (name, nlock, len(prns)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
