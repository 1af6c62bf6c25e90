"""What C/N0 does every satellite have in the IQ a receiver is handed?  RINEX file -> front end -> a chained batch on the GPU ->
gpsbb_batch_despread in the view of each output format (SC16, SC8 at a shift, SC1) with the library's noise at a chosen C/N0 ->
per PRN: the C/N0 asked for scaled by the channel's gain, the C/N0 realised (gpsbb_cn0_estimate over the whole segments), the loss.

    python tools/cn0_report.py [-e tests/golden/synth3540.14n] [-W cn0[,shift]] [-q sc8_shift] [-s fs] [-d seconds] [-t seg_tiles] [-o OUT]

-W as gpsbb-sim's: C/N0 in dB-Hz of a gain-1.0 channel and the noise shift (default 45,0).  -q: SC8's shift (default: the one
that puts the noise's sigma just under 64 int8 counts).  Default output: profiles/ds01_cn0_report.txt.
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
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-e", default=os.path.join(ROOT, "tests", "golden", "synth3540.14n"))
    ap.add_argument("-W", default="45,0")
    ap.add_argument("-q", type=int, default=-1)
    ap.add_argument("-s", type=float, default=2.6e6)
    ap.add_argument("-d", type=float, default=1.0)
    ap.add_argument("-t", type=int, default=2)
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "ds01_cn0_report.txt"))
    a = ap.parse_args()
    cn0 = float(a.W.split(",")[0])
    nshift = int(a.W.split(",")[1]) if "," in a.W else 0
    fs, delt = a.s, 1.0 / a.s
    nsamp = int(round(fs * 0.1))   # the front end's blocks are 0.1 s (the reference's)
    nblocks = max(2, int(round(a.d * 10)))
    fe = pkg.FrontEnd(a.e, llh=(30.286502, 120.032669, 100.0), max_chan=12)
    ch = fe.generate(nblocks)
    fe.close()
    sigma = pkg.noise_sigma(cn0, 1.0, delt)
    shift8 = a.q if a.q >= 0 else max(0, math.ceil(math.log2(sigma / (1 << nshift) / 64.0)))
    nz = pkg.Noise(1, 0, sigma, nshift, 0)
    whole_per_block = nsamp // (1024 * a.t)
    T = 1024 * a.t * delt
    views = (("sc16", pkg.OUT_SC16), ("sc8>>%d" % shift8, pkg.OUT_SC8(shift8)), ("sc1", pkg.OUT_SC1))
    with pkg.Synth(0) as s:
        b = s.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
        b.run()
        s.sync()
        variant = s.info(pkg.INFO_LAST_VARIANT)
        sums = {name: b.despread(view=fmt, noise=nz, seg_tiles=a.t) for name, fmt in views}
        b.close()
    lines = ["# %s, %.4g MS/s, %d blocks of %d samples (%.1f s), 12 channel slots, synthesis kernel variant %d"
             % (os.path.basename(a.e), fs / 1e6, nblocks, nsamp, nblocks * 0.1, variant),
             "# noise: %.1f dB-Hz for a gain-1.0 channel (sigma %.1f per component, shift %d), segments of %d tiles (%.3f ms), %d whole per block"
             % (cn0, sigma, nshift, a.t, T * 1e3, whole_per_block),
             "# PRN  blocks  gain   asked   " + "   ".join("%-8s loss " % n for n, _ in views)]
    for i in range(ch.shape[1]):
        # a channel slot may change hands: one line per PRN it carried
        for prn in sorted(set(int(p) for p in ch["prn"][:, i] if p > 0)):
            blocks = np.nonzero(ch["prn"][:, i] == prn)[0]
            if blocks.size * whole_per_block < 2:
                continue
            gain = float(np.sqrt(np.mean(ch["gain"][blocks, i] ** 2)))
            asked = cn0 + 20 * math.log10(gain)
            row = "%5d %7d %6.3f %7.2f" % (prn, blocks.size, gain, asked)
            for name, _ in views:
                p = np.ascontiguousarray(sums[name][blocks, i, :whole_per_block].reshape(-1, 2))
                got = pkg.cn0_estimate(p, T)
                row += "   %8.2f %+5.2f" % (got, got - asked)
            lines.append(row)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
