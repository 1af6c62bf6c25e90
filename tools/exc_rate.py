"""What the excision costs: gpsbb_device_excise over 25 000 000 resident int16 IQ samples at every log2n, under gpsbb_exc_make's
window with a tenth of the bins masked and no threshold, plain and with noise — milliseconds per call (the kernels by HIP events:
the experiments build's gpsbb_test_exc_ms; the whole synchronous call by the host's clock), the median of five, samples per second,
and the kernel's share of the HBM floor of 8 bytes per sample (4 read, 4 written) at HBM_BYTES_PER_S.  Beside it on the same
buffer: gpsbb_device_psd under Hann at hop N / 2, which does the forward half of the work on the same segments.  No threshold on
the figures: they go on record.

    GPSBB_PY_LIB=exp python tools/exc_rate.py [--json OUT] [--quick]     (env: REPEATS=5)
Default output: profiles/ex01_exc_rate.json.
"""
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPSBB_PY_LIB", "exp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)

from __graft_entry__ import load_package  # noqa: E402
import exc_check as ec  # noqa: E402

pkg = load_package()

repeats = int(os.environ.get("REPEATS", "5"))
quick = "--quick" in sys.argv
L = pkg.lib()
if not hasattr(L, "gpsbb_test_exc_ms"):
    sys.exit("the experiments build is wanted (GPSBB_PY_LIB=exp): the kernels' time comes from its hook")
for fn in (L.gpsbb_test_exc_ms, L.gpsbb_test_psd_ms):
    fn.argtypes = [pkg.C.c_void_p]
    fn.restype = pkg.C.c_float

HBM_BYTES_PER_S = 8.0e12   # MI355X: 8 TB/s peak
noise = {"seed": 0xE5D, "sample0": (1 << 32) + 12345, "sigma": 700.0, "shift": 1}
NSAMP = 2500000 if quick else 25000000


def timed(call, hook):
    call()   # warm: the scratch, the tables, the noise table
    ms, wall = [], []
    for _ in range(1 if quick else repeats):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(hook()))
    return statistics.median(ms), min(ms), max(ms), statistics.median(wall)


out = {"tool": "exc_rate", "repeats": repeats, "quick": quick, "hbm_bytes_per_s": HBM_BYTES_PER_S, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
       "legs": []}
with pkg.Synth(0) as s:
    src = torch.randint(-8000, 8000, (NSAMP, 2), dtype=torch.int16, device="cuda")
    dst = torch.zeros((NSAMP, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for log2n in ec.LOG2NS:
        N, H = 1 << log2n, 1 << (log2n - 1)
        nsamp = NSAMP // H * H
        floor_ms = nsamp * 8 / HBM_BYTES_PER_S * 1e3
        e = pkg.exc_make(log2n).copy(bins=ec.random_bins(N, 0.1, 0xE900 + log2n))
        for name, nz in (("plain", None), ("noise", noise)):
            m, lo, hi, wall = timed(lambda: s.device_excise(src.data_ptr(), nsamp, e, dst.data_ptr(), None, nz), lambda: L.gpsbb_test_exc_ms(s._h))
            leg = {"call": "excise", "nsamp": nsamp, "n": N, "view": name, "kernel_ms": m, "kernel_ms_min": lo, "kernel_ms_max": hi, "call_ms": wall,
                   "samples_per_s": nsamp / (m * 1e-3), "hbm_floor_ms": floor_ms, "share_of_hbm_floor": floor_ms / m}
            print("excise %8d samples N %4d %-5s kernels %8.3f ms (%.3f .. %.3f), call %8.3f ms: %.3g samples per s, %.1f %% of the floor"
                  % (nsamp, N, name, m, lo, hi, wall, leg["samples_per_s"], 100 * leg["share_of_hbm_floor"]), flush=True)
            out["legs"].append(leg)
        p = pkg.psd_make(log2n, nsamp, 0, pkg.PSD_HANN)
        m, lo, hi, wall = timed(lambda: s.device_psd(src.data_ptr(), nsamp, p), lambda: L.gpsbb_test_psd_ms(s._h))
        print("psd    %8d samples N %4d hann  plain kernels %8.3f ms (%.3f .. %.3f), call %8.3f ms" % (nsamp, N, m, lo, hi, wall), flush=True)
        out["legs"].append({"call": "psd", "nsamp": nsamp, "n": N, "window": "hann", "hop": int(p.hop), "view": "plain", "kernel_ms": m, "kernel_ms_min": lo,
                            "kernel_ms_max": hi, "call_ms": wall})

print(json.dumps(out))
dst_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "ex01_exc_rate.json")
with open(dst_path, "w") as f:
    json.dump(out, f, indent=1)
