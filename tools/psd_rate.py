"""What the power spectrum costs: gpsbb_device_psd over resident int16 IQ of 2 500 000 and 25 000 000 samples, N = 256, 1024 and
4096, under the rectangular window (hop N: every sample read once) and Hann (hop N / 2), SC16 plain and with noise — milliseconds
per call (the kernels by HIP events: the experiments build's gpsbb_test_psd_ms; the whole synchronous call by the host's clock), the
median of five, input samples per second, and the kernel's share of the HBM read floor (4 bytes per sample at HBM_BYTES_PER_S).
Beside it on the same buffer: k_fir plain (fir_make(33, 4)), and what the call replaces, reading the buffer back (device_read).
No threshold: the figures go on record.

    GPSBB_PY_LIB=exp python tools/psd_rate.py [--json OUT] [--quick]     (env: REPEATS=5)
Default output: profiles/ps01_psd_rate.json.
"""
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
os.environ.setdefault("GPSBB_PY_LIB", "exp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()

repeats = int(os.environ.get("REPEATS", "5"))
quick = "--quick" in sys.argv
L = pkg.lib()
if not hasattr(L, "gpsbb_test_psd_ms"):
    sys.exit("the experiments build is wanted (GPSBB_PY_LIB=exp): the kernels' time comes from its hook")
for fn in (L.gpsbb_test_psd_ms, L.gpsbb_test_fir_ms):
    fn.argtypes = [pkg.C.c_void_p]
    fn.restype = pkg.C.c_float

HBM_BYTES_PER_S = 8.0e12   # MI355X: 8 TB/s peak
noise = {"seed": 0x95D, "sample0": (1 << 32) + 12345, "sigma": 700.0, "shift": 1}
sizes = (2500000,) if quick else (2500000, 25000000)


def timed(call, hook):
    call()   # warm: the scratch, the noise table
    ms, wall = [], []
    for _ in range(1 if quick else repeats):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(hook()) if hook else float("nan"))
    return statistics.median(ms), min(ms), max(ms), statistics.median(wall)


out = {"tool": "psd_rate", "repeats": repeats, "quick": quick, "hbm_bytes_per_s": HBM_BYTES_PER_S, "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"],
       "legs": []}
with pkg.Synth(0) as s:
    for nsamp in sizes:
        src = torch.randint(-8000, 8000, (nsamp, 2), dtype=torch.int16, device="cuda")
        dst = torch.zeros((nsamp // 4, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        floor_ms = nsamp * 4 / HBM_BYTES_PER_S * 1e3
        for log2n in (8, 10, 12):
            for wname, window in (("rect", pkg.PSD_RECT), ("hann", pkg.PSD_HANN)):
                p = pkg.psd_make(log2n, nsamp, 0, window)
                for name, nz in (("plain", None), ("noise", noise)):
                    m, lo, hi, wall = timed(lambda: s.device_psd(src.data_ptr(), nsamp, p, pkg.OUT_SC16, nz), lambda: L.gpsbb_test_psd_ms(s._h))
                    leg = {"call": "psd", "nsamp": nsamp, "n": 1 << log2n, "window": wname, "hop": int(p.hop), "shift": int(p.shift),
                           "nseg": pkg.psd_nseg(p, nsamp), "view": name, "kernel_ms": m, "kernel_ms_min": lo, "kernel_ms_max": hi, "call_ms": wall,
                           "input_samples_per_s": nsamp / (m * 1e-3), "hbm_read_floor_ms": floor_ms, "share_of_hbm_read_floor": floor_ms / m}
                    print("psd  %8d samples N %4d %-4s %-5s kernels %8.3f ms (%.3f .. %.3f), call %8.3f ms: %.3g samples per s, %.1f %% of the read floor"
                          % (nsamp, 1 << log2n, wname, name, m, lo, hi, wall, leg["input_samples_per_s"], 100 * leg["share_of_hbm_read_floor"]), flush=True)
                    out["legs"].append(leg)
        fir = pkg.fir_make(33, 4)
        m, lo, hi, wall = timed(lambda: s.device_fir(src.data_ptr(), nsamp, fir, dst.data_ptr()), lambda: L.gpsbb_test_fir_ms(s._h))
        print("fir  %8d samples (33, 4) plain  kernel %8.3f ms (%.3f .. %.3f), call %8.3f ms" % (nsamp, m, lo, hi, wall), flush=True)
        out["legs"].append({"call": "fir", "nsamp": nsamp, "ntaps": 33, "decim": 4, "view": "plain", "kernel_ms": m, "kernel_ms_min": lo, "kernel_ms_max": hi,
                            "call_ms": wall, "share_of_hbm_read_floor": floor_ms / m})
        _, _, _, wall = timed(lambda: s.device_read(src.data_ptr(), (nsamp, 2)), None)
        print("read %8d samples back to the host: %8.3f ms" % (nsamp, wall), flush=True)
        out["legs"].append({"call": "device_read", "nsamp": nsamp, "call_ms": wall, "bytes": nsamp * 4})
        del src, dst

print(json.dumps(out))
dst_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "ps01_psd_rate.json")
with open(dst_path, "w") as f:
    json.dump(out, f, indent=1)
