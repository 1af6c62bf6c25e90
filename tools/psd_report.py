"""Where does the power of a scenario sit in frequency, in the IQ a receiver is handed?  RINEX file -> front end -> one block
rendered on the GPU -> gpsbb_device_psd (Hann, N = 1 << -n) in the view of each output format (SC16, SC8 at a shift, SC1) with
the library's noise (-W) and emitters (-J) fused by stream position: the spectrum in dB per bin, relative to the view's own mean
square (0 dB: a bin that holds 1 / N of the power), frequency ascending.  With -D the block is rendered at -s times decim and the
spectrum is taken before the front-end filter (at the rendered rate) and after gpsbb_device_fir (at -s): the stop band and what
aliases through it are there to see.

    python tools/psd_report.py [-e tests/golden/synth3540.14n] [-W cn0[,shift]] [-J cw,js_db,f_hz | chirp,js_db,f0_hz,f1_hz,sweep_s]...
                               [-D decim[,ntaps]] [-q sc8_shift] [-s fs] [-d seconds] [-n log2n] [-b bins_per_line] [-o OUT]

-W and -J as gpsbb-sim's (without the pulse fields).  Default output: profiles/ps01_psd_report.txt.
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


def emitter(spec, delt):
    f = spec.split(",")
    if f[0] == "cw":
        return pkg.interf_make(pkg.INTERF_CW, float(f[1]), float(f[2]), delt=delt)
    return pkg.interf_make(pkg.INTERF_CHIRP, float(f[1]), float(f[2]), float(f[3]), float(f[4]), delt=delt)


def db_lines(name, fs, p, nseg, psd, view, per_line):
    """the bins in dB against the mean bin, frequency ascending (bins from N / 2 first: they are the negative frequencies)"""
    N = psd.size
    x = psd.astype(np.float64) * pkg.psd_scale(p, nseg, view)
    total = x.sum()
    db = 10.0 * np.log10(np.maximum(x * N / max(total, 1e-300), 1e-30))
    order = np.r_[np.arange(N // 2, N), np.arange(0, N // 2)]
    freq = (order - np.where(order >= N // 2, N, 0)) * fs / N
    step = max(1, N // per_line)
    out = ["%-14s mean square %.6g (view units), %d segments, shift %d, largest bin at %+.1f kHz: %.1f dB"
           % (name, total, nseg, p.shift, freq[int(np.argmax(db[order]))] / 1e3, db.max())]
    for i in range(0, N, step):   # the strongest bin of every group: a tone is not averaged away
        j = i + int(np.argmax(db[order][i:i + step]))
        out.append("  %+10.1f kHz %8.2f dB" % (freq[j] / 1e3, db[order][j]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-e", default=os.path.join(ROOT, "tests", "golden", "synth3540.14n"))
    ap.add_argument("-W", default="")
    ap.add_argument("-J", action="append", default=[])
    ap.add_argument("-D", default="")
    ap.add_argument("-q", type=int, default=-1)
    ap.add_argument("-s", type=float, default=2.6e6)
    ap.add_argument("-d", type=float, default=0.1)
    ap.add_argument("-n", type=int, default=10)
    ap.add_argument("-b", type=int, default=64)
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "ps01_psd_report.txt"))
    a = ap.parse_args()
    D = int(a.D.split(",")[0]) if a.D else 1
    T = int(a.D.split(",")[1]) if "," in a.D else 8 * D + 1
    fs_in, delt = a.s * D, 1.0 / (a.s * D)
    nsamp = int(round(fs_in * a.d)) // D * D
    nshift = int(a.W.split(",")[1]) if "," in a.W else 0
    nz = pkg.Noise(1, 0, pkg.noise_sigma(float(a.W.split(",")[0]), 1.0, delt), nshift, 0) if a.W else None
    js = pkg.InterfSet([emitter(s, delt) for s in a.J], nshift, 0) if a.J else None
    fe = pkg.FrontEnd(a.e, llh=(30.286502, 120.032669, 100.0), max_chan=12)
    ch = fe.generate(1)
    fe.close()
    lines = ["# %s, %.4g MS/s%s, one block of %d samples; noise %s; emitters %s; Hann, N = %d" % (
        os.path.basename(a.e), a.s / 1e6, " rendered at %.4g MS/s" % (fs_in / 1e6) if D > 1 else "", nsamp, a.W or "none", " ".join(a.J) or "none", 1 << a.n),
        "# dB relative to the mean bin of the same spectrum; of every %d bins the strongest" % max(1, (1 << a.n) // a.b)]
    with pkg.Synth(0) as s:
        b = s.batch(ch, delt, nsamp)
        b.run()
        s.sync()
        d_iq = b.device_iq()
        p = pkg.psd_make(a.n, nsamp, 0, pkg.PSD_HANN)
        if D == 1:
            lv = s.device_level(d_iq, 1, nsamp, nz, js)
            rms = math.sqrt(float(lv["sumsq"].sum()) / (2.0 * nsamp)) / (1 << nshift)
            shift8 = a.q if a.q >= 0 else max(0, math.ceil(math.log2(max(rms, 1.0) / 32.0)))
            for name, view in (("sc16", pkg.OUT_SC16), ("sc8>>%d" % shift8, pkg.OUT_SC8(shift8)), ("sc1", pkg.OUT_SC1)):
                psd, nseg = s.device_psd(d_iq, nsamp, p, view, nz, js)
                lines += db_lines(name, a.s, p, nseg, psd, view, a.b)
        else:
            import torch
            fir = pkg.fir_make(T, D)
            dst = torch.zeros((nsamp // D, 2), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            psd, nseg = s.device_psd(d_iq, nsamp, p, pkg.OUT_SC16, nz, js)
            lines += db_lines("before -D", fs_in, p, nseg, psd, pkg.OUT_SC16, a.b)
            _, clipped = s.device_fir(d_iq, nsamp, fir, dst.data_ptr(), None, nz, js)
            q = pkg.psd_make(a.n, nsamp // D, 0, pkg.PSD_HANN)
            psd, nseg = s.device_psd(dst.data_ptr(), nsamp // D, q)
            lines += db_lines("after -D %d,%d" % (D, T), a.s, q, nseg, psd, pkg.OUT_SC16, a.b)
            lines.append("# the filter clipped %d components" % clipped)
        b.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
