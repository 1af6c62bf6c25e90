"""What does multipath do to the correlation function a receiver forms?  RINEX file + echoes -> front end -> a chained batch on
the GPU -> gpsbb_batch_despread_lags in the view of each output format (SC16, SC8 at a shift, SC1) with the library's noise at
a chosen C/N0 -> per PRN: |P(L)| / |P(0)| over a lag range, P summed over the whole run.  tools/cn0_report.py's parts with one
more axis.

    python tools/lag_profile.py [-e tests/golden/synth3540.14n] -M prn,extra_m,atten_db[,phase_cyc[,rate_mps]] [-M ...]
                                [-L lo,hi] [-W cn0[,shift]] [-q sc8_shift] [-s fs] [-d seconds] [-o OUT]

-M as gpsbb-sim's, up to eight times.  -L: the lag range in samples (default -4,11; any length within +-64: the call takes eight
lags at a time).  Default output: profiles/mp01_lag_profile.txt.
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
    ap.add_argument("-M", action="append", default=[])
    ap.add_argument("-L", default="-4,11")
    ap.add_argument("-W", default="45,0")
    ap.add_argument("-q", type=int, default=-1)
    ap.add_argument("-s", type=float, default=2.6e6)
    ap.add_argument("-d", type=float, default=1.0)
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "mp01_lag_profile.txt"))
    a = ap.parse_args()
    cn0 = float(a.W.split(",")[0])
    nshift = int(a.W.split(",")[1]) if "," in a.W else 0
    lo, hi = [int(v) for v in a.L.split(",")]
    lags = list(range(lo, hi + 1))
    if 0 not in lags:
        ap.error("-L must include lag 0")
    echoes = [tuple(float(v) for v in m.split(",")) for m in a.M]
    fs, delt = a.s, 1.0 / a.s
    nsamp = int(round(fs * 0.1))   # the front end's blocks are 0.1 s (the reference's)
    nblocks = max(1, int(round(a.d * 10)))
    pkg.build_frontend()
    fe = pkg.FrontEnd(a.e, llh=(30.286502, 120.032669, 100.0), max_chan=12 if len(echoes) <= 4 else 16 - len(echoes))
    max_chan = fe.max_chan
    fe.set_echoes(echoes)
    ch = fe.generate(nblocks)
    fe.close()
    sigma = pkg.noise_sigma(cn0, 1.0, delt)
    shift8 = a.q if a.q >= 0 else max(0, math.ceil(math.log2(sigma / (1 << nshift) / 64.0)))
    nz = pkg.Noise(1, 0, sigma, nshift, 0)
    views = (("sc16", pkg.OUT_SC16), ("sc8>>%d" % shift8, pkg.OUT_SC8(shift8)), ("sc1", pkg.OUT_SC1))
    ntiles = -(-nsamp // 1024)
    with pkg.Synth(0) as s:
        b = s.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
        b.run()
        s.sync()
        variant = s.info(pkg.INFO_LAST_VARIANT)
        sums = {}
        for name, fmt in views:   # eight lags a call; one segment per block
            parts = [b.despread_lags(lags[k:k + 8], seg_tiles=ntiles, view=fmt, noise=nz) for k in range(0, len(lags), 8)]
            sums[name] = np.concatenate(parts, axis=3)[:, :, 0]
        b.close()
    lines = ["# %s, %.4g MS/s, %d blocks of %d samples, %d channel slots + %d echoes, synthesis kernel variant %d"
             % (os.path.basename(a.e), fs / 1e6, nblocks, nsamp, max_chan, len(echoes), variant),
             "# noise: %.1f dB-Hz for a gain-1.0 channel (sigma %.1f per component, shift %d); |P(L)| / |P(0)|, P summed over the run"
             % (cn0, sigma, nshift)]
    for j, e in enumerate(echoes):
        lines.append("# echo %d: PRN %d, %.1f m (%.2f samples), %.1f dB down" % (j, int(e[0]), e[1], e[1] / 2.99792458e8 * fs, e[2]))
    lines.append("# PRN view      " + " ".join("%6d" % v for v in lags))
    for i in range(max_chan):
        for prn in sorted(set(int(p) for p in ch["prn"][:, i] if p > 0)):
            blocks = np.nonzero(ch["prn"][:, i] == prn)[0]
            for name, _ in views:
                p = sums[name][blocks, i].sum(axis=0).astype(np.float64)   # [lag, i/q]
                mag = np.hypot(p[:, 0], p[:, 1])
                lines.append("%5d %-8s " % (prn, name) + " ".join("%6.3f" % (m / mag[lags.index(0)]) for m in mag))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
