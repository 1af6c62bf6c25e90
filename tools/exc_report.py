"""What excision buys a receiver: tools/acq_check.py's six satellites and search plan at 2.6 MS/s, 8192 samples rendered on the GPU
under tools/exc_check.py's noise, with a CW emitter and with the full-band chirp at a list of J/S — per PRN whether the search finds
its cell and the C/N0 its peak implies, on the impaired view (gpsbb_device_acquire with the emitter fused) and on the output of
gpsbb_device_excise at N = 256 (the plan from gpsbb_device_psd and gpsbb_exc_from_psd, as tests/test_excise_gpu.py makes it).

The C/N0 is read off the search's own figure: gpsbb_acq_best's ratio is the peak over the mean cell of the PRN's grid, so with a
coherent time T the peak implies C/N0 = 10 log10(max(ratio - 1, 0) / T) dB-Hz; below about 36 dB-Hz it is the floor's own
largest cell that speaks.  Every excised output is compared == with the numpy mirror on the way.

    python tools/exc_report.py [--js 10,20,30,35] [--out profiles/ex01_exc_report.txt]
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (one HIP runtime for torch and libgpsbb)

from __graft_entry__ import load_package  # noqa: E402
import exc_check as ec  # noqa: E402
from exc_check import ac  # noqa: E402

T_COH = 1e-3


def cn0(ratio):
    return 10.0 * math.log10(max(ratio - 1.0, 1e-9) / T_COH)


def per_prn(pkg, rows, cfg, ch):
    bad, present, _ = ac.e2e_findings(pkg, rows, cfg, ch)
    wrong = {int(f.split()[1].rstrip(":")) for f in bad if f.startswith("PRN")}
    return {p: (p not in wrong, cn0(r)) for p, r in present.items()}


def main():
    args = sys.argv[1:]
    levels = [float(v) for v in (args[args.index("--js") + 1] if "--js" in args else "10,20,30,35").split(",")]
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "ex01_exc_report.txt")
    pkg = load_package()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with pkg.Synth(0) as s:
        ch = ec.e2e_descriptors(pkg)
        n, H = ec.E2E_NSAMP, ec.E2E_H
        b = s.batch(ch, 1.0 / ec.FS, n)
        b.run()
        s.sync()
        iq, d_iq = b.read()[0][0], b.device_iq()
        cfg = ac.e2e_cfg(pkg, pkg.OUT_SC16)
        pp = ec.e2e_psd_plan(pkg)
        quiet = per_prn(pkg, s.device_acquire(d_iq, ac.E2E_NSAMP, cfg, pkg.OUT_SC16, ec.E2E_NOISE), cfg, ch)
        say("six satellites at 2.6 MS/s, noise sigma %g at shift %d, N = %d; C/N0 in dB-Hz, * where the search finds the PRN's cell"
            % (ec.E2E_NOISE["sigma"], ec.E2E_NOISE["shift"], ec.E2E_N))
        say("no emitter:            " + "  ".join("PRN %d %5.1f%s" % (p, c, "*" if ok else " ") for p, (ok, c) in quiet.items()))
        out = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
        for kind, make in (("cw", ec.cw_set), ("chirp", ec.sweep_set)):
            for js_db in levels:
                js = make(pkg, js_db)
                before = per_prn(pkg, s.device_acquire(d_iq, ac.E2E_NSAMP, cfg, pkg.OUT_SC16, ec.E2E_NOISE, js), cfg, ch)
                spectrum, nseg = s.device_psd(d_iq, n, pp, pkg.OUT_SC16, ec.E2E_NOISE, js if kind == "cw" else None)
                e = ec.e2e_plan(pkg, spectrum, nseg, pp, kind)
                hist, clipped, excised = s.device_excise(d_iq, n, e, out.data_ptr(), None, ec.E2E_NOISE, js)
                bad = ec.compare((out.cpu().numpy(), hist, clipped, excised), ec.mirror(pkg, iq, e, None, ec.E2E_NOISE, js), kind)
                after = per_prn(pkg, s.device_acquire(out.data_ptr() + 4 * H, ac.E2E_NSAMP, cfg), cfg, ch)
                say("%-5s J/S %4.1f dB before: " % (kind, js_db) + "  ".join("PRN %d %5.1f%s" % (p, c, "*" if ok else " ") for p, (ok, c) in before.items()))
                say("%-5s J/S %4.1f dB after:  " % (kind, js_db) + "  ".join("PRN %d %5.1f%s" % (p, c, "*" if ok else " ") for p, (ok, c) in after.items())
                    + "   (%d bins masked, thr %d, %.1f %% of the cells zeroed, %d clipped%s)" % (
                        int(e.bins().sum()), int(e.thr), 100.0 * excised / (n // H * ec.E2E_N), clipped, "" if not bad else "; NOT the mirror: " + "; ".join(bad)))
        b.close()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
