"""What does a jammer cost every satellite in the IQ a receiver is handed?  RINEX file -> front end -> a chained batch on the GPU ->
gpsbb_batch_despread_impaired in the view of each output format (SC16, SC8 at a shift, SC1), the library's noise at a chosen C/N0
plus one emitter at each of a list of J/S values -> per PRN and J/S: the C/N0 realised (gpsbb_cn0_estimate over the whole segments).

    python tools/jam_report.py [-e tests/golden/synth3540.14n] [-W cn0[,shift]] [-J chirp,f0_hz,f1_hz,sweep_s | cw,f_hz]
                               [-L js_db,js_db,...] [-q sc8_shift] [-s fs] [-d seconds] [-t seg_tiles] [-o OUT]

-W as gpsbb-sim's (default 45,1).  -J without its J/S: the emitter (default: a chirp over the whole band in 2048 samples).  -L: the
J/S values in dB against a gain-1.0 channel (default 0,10,20,30).  Default output: profiles/jm01_jam_report.txt.
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
    ap.add_argument("-W", default="45,1")
    ap.add_argument("-J", default="")
    ap.add_argument("-L", default="0,10,20,30")
    ap.add_argument("-q", type=int, default=-1)
    ap.add_argument("-s", type=float, default=2.6e6)
    ap.add_argument("-d", type=float, default=1.0)
    ap.add_argument("-t", type=int, default=2)
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "jm01_jam_report.txt"))
    a = ap.parse_args()
    cn0 = float(a.W.split(",")[0])
    nshift = int(a.W.split(",")[1]) if "," in a.W else 0
    fs, delt = a.s, 1.0 / a.s
    nsamp = int(round(fs * 0.1))
    nblocks = max(2, int(round(a.d * 10)))
    spec = a.J.split(",") if a.J else ["chirp", str(-fs / 2), str(fs / 2), repr(2048 * delt)]
    levels = [float(x) for x in a.L.split(",")]

    def emitter(js_db):
        if spec[0] == "cw":
            return pkg.interf_make(pkg.INTERF_CW, js_db, float(spec[1]), delt=delt)
        return pkg.interf_make(pkg.INTERF_CHIRP, js_db, float(spec[1]), float(spec[2]), float(spec[3]), delt=delt)

    fe = pkg.FrontEnd(a.e, llh=(30.286502, 120.032669, 100.0), max_chan=12)
    ch = fe.generate(nblocks)
    fe.close()
    sigma = pkg.noise_sigma(cn0, 1.0, delt)
    shift8 = a.q if a.q >= 0 else max(0, math.ceil(math.log2(sigma / (1 << nshift) / 64.0)))
    nz = pkg.Noise(1, 0, sigma, nshift, 0)
    whole_per_block = nsamp // (1024 * a.t)
    T = 1024 * a.t * delt
    views = (("sc16", pkg.OUT_SC16), ("sc8>>%d" % shift8, pkg.OUT_SC8(shift8)), ("sc1", pkg.OUT_SC1))
    sums = {}
    with pkg.Synth(0) as s:
        b = s.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
        b.run()
        s.sync()
        for name, fmt in views:
            sums[name, None] = b.despread(view=fmt, noise=nz, seg_tiles=a.t)
            for js_db in levels:
                sums[name, js_db] = b.despread(view=fmt, noise=nz, seg_tiles=a.t, interf=pkg.InterfSet([emitter(js_db)], nshift, 0))
        b.close()
    cols = [None] + levels
    lines = ["# %s, %.4g MS/s, %d blocks of %d samples (%.1f s), 12 channel slots" % (os.path.basename(a.e), fs / 1e6, nblocks, nsamp, nblocks * 0.1),
             "# noise: %.1f dB-Hz for a gain-1.0 channel (sigma %.1f per component, shift %d); emitter: %s; segments of %d tiles (%.3f ms)"
             % (cn0, sigma, nshift, ",".join(spec), a.t, T * 1e3),
             "# C/N0 found (dB-Hz) per J/S in dB against a gain-1.0 channel",
             "# view     PRN   gain  asked " + " ".join("%7s" % ("none" if c is None else "%+.0f" % c) for c in cols)]
    for name, _ in views:
        for i in range(ch.shape[1]):
            for prn in sorted(set(int(p) for p in ch["prn"][:, i] if p > 0)):
                blocks = np.nonzero(ch["prn"][:, i] == prn)[0]
                if blocks.size * whole_per_block < 2:
                    continue
                gain = float(np.sqrt(np.mean(ch["gain"][blocks, i] ** 2)))
                row = "%-8s %5d %6.3f %6.2f" % (name, prn, gain, cn0 + 20 * math.log10(gain))
                for c in cols:
                    p = np.ascontiguousarray(sums[name, c][blocks, i, :whole_per_block].reshape(-1, 2))
                    row += " %7.2f" % pkg.cn0_estimate(p, T)
                lines.append(row)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
