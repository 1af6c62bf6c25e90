"""What does the front-end filter do to a receiver's code loop?  The end-to-end scenario of the tests (tools/fir_check.py: six
satellites, 0.5 s) tracked twice by the existing chain — once from a direct render at 2.6 MS/s, whose chips are point-sampled on a
385 ns grid, once from a render at 10.4 MS/s band-limited and decimated to 2.6 MS/s by gpsbb_device_fir with fir_make(33, 4) — and per
PRN, over the records after the pull-in: the RMS of the code discriminator e_d, and the tracked code phase at each epoch's first
sample against the descriptor's (code_phase + f_code * delt * n0, in chips): its mean (the filter's delay shows here: 3.25 output
samples, 1.28 chips) and its RMS about the mean.  It prints only; no figure is promised.

    python tools/fir_report.py [-k skip] [-o OUT]
Default output: profiles/fr01_fir_report.txt.
"""
import argparse
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)
import numpy as np  # noqa: E402

import fir_check as fc  # noqa: E402
import track_check as tc  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()


def chain(s, d_iq):
    acq, trk = tc.e2e_acq_cfg(pkg, pkg.OUT_SC16), tc.e2e_trk_cfg(pkg)
    rows = s.device_acquire(d_iq, tc.E2E_ACQ_NSAMP, acq)
    return s.device_track(d_iq, tc.E2E_NSAMP, trk, tc.e2e_seeds(pkg, rows, acq))[1]


def code_error(d, r, skip):
    """the tracked code phase minus the descriptor's at each record's first sample, in chips, wrapped to +-511.5"""
    n0 = r["n0"][skip:].astype(np.float64)
    truth = float(d["code_phase"]) + float(d["f_code"]) / fc.FS * n0
    e = r["code_phase"][skip:].astype(np.float64) / float(1 << 32) - truth
    return (e + 511.5) % 1023.0 - 511.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, default=tc.E2E_SKIP)
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "fr01_fir_report.txt"))
    a = ap.parse_args()
    ch = tc.e2e_descriptors(pkg)
    fir = fc.e2e_fir(pkg)
    out = {}
    with pkg.Synth(0) as s:
        b = s.batch(ch, 1.0 / fc.FS, tc.E2E_NSAMP)
        b.run()
        s.sync()
        out["direct"] = chain(s, b.device_iq())
        b.close()
        dec = torch.zeros((tc.E2E_NSAMP, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        b = s.batch(ch, 1.0 / fc.FS_IN, fc.E2E_NSAMP_IN)
        b.run()
        s.sync()
        _, clipped = s.device_fir(b.device_iq(), fc.E2E_NSAMP_IN, fir, dec.data_ptr())
        out["decimated"] = chain(s, dec.data_ptr())
        b.close()
    lines = ["# six satellites (synth_descriptors seed 0xACC), %d samples at 2.6 MS/s: rendered directly, and rendered at 10.4 MS/s then"
             % tc.E2E_NSAMP,
             "# filtered by fir_make(%d, %d) (shift %d, clipped %d); records from %d on" % (fir.ntaps, fir.decim, fir.shift, clipped, a.k),
             "# stream     PRN   gain  records  rms e_d   code error: mean (chips)  rms about the mean (chips)"]
    for name in ("direct", "decimated"):
        for k, prn in enumerate(tc.E2E_PRESENT):
            d, r = ch[0, prn - 1], out[name][k]
            if r.size <= a.k + 10:
                lines.append("%-10s %4d: %d records" % (name, prn, r.size))
                continue
            e = code_error(d, r, a.k)
            lines.append("%-10s %4d %6.3f %8d %8.1f %24.4f %27.4f"
                         % (name, prn, float(d["gain"]), r.size, float(np.sqrt(np.mean(r["e_d"][a.k:].astype(np.float64) ** 2))), float(e.mean()),
                            float(e.std())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
