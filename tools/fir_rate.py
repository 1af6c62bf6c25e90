"""What the front-end filter costs: gpsbb_device_fir over one resident render of six satellites, 0.1 s at 25 MS/s (2 500 000 input
samples), for (T, D) = (33, 4), (65, 8), (129, 16), each plain, with noise, and with noise and a chirp — milliseconds per call (the
kernel by HIP events: the experiments build's gpsbb_test_fir_ms; the whole synchronous call by the host's clock), the median of
five, and input samples per second.  No threshold: the figures go on record.

    GPSBB_PY_LIB=exp python tools/fir_rate.py [--json OUT] [--quick]     (env: REPEATS=5)
Default output: profiles/fr01_fir_rate.json.
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
if not hasattr(L, "gpsbb_test_fir_ms"):
    sys.exit("the experiments build is wanted (GPSBB_PY_LIB=exp): the kernel's time comes from its hook")
L.gpsbb_test_fir_ms.argtypes = [pkg.C.c_void_p]
L.gpsbb_test_fir_ms.restype = pkg.C.c_float

FS = 25e6
delt = 1.0 / FS
nsamp = 2400000 if quick else 2500000   # a multiple of 16
noise = {"seed": 0xF1A, "sample0": (1 << 32) + 12345, "sigma": 700.0, "shift": 1}
chirp = pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -0.2 * FS, 0.27 * FS, 301 * delt, delt=delt)], noise["shift"], noise["sample0"])

out = {"tool": "fir_rate", "repeats": repeats, "quick": quick, "fs": FS, "nsamp": nsamp, "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"],
       "legs": []}
with pkg.Synth(0) as s:
    ch = pkg.synth_descriptors(1, nch=6, seed=0xACC)
    b = s.batch(ch, delt, nsamp)
    b.run()
    s.sync()
    dst = torch.zeros((nsamp, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for T, D in ((33, 4), (65, 8), (129, 16)):
        fir = pkg.fir_make(T, D)
        for name, nz, js in (("plain", None, None), ("noise", noise, None), ("noise+chirp", noise, chirp)):
            s.device_fir(b.device_iq(), nsamp, fir, dst.data_ptr(), None, nz, js)   # warm: the scratch, the noise table
            ms, wall = [], []
            for _ in range(1 if quick else repeats):
                t0 = time.perf_counter()
                s.device_fir(b.device_iq(), nsamp, fir, dst.data_ptr(), None, nz, js)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(float(L.gpsbb_test_fir_ms(s._h)))
            m = statistics.median(ms)
            leg = {"ntaps": T, "decim": D, "view": name, "kernel_ms": m, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                   "call_ms": statistics.median(wall), "input_samples_per_s": nsamp / (m * 1e-3),
                   "input_samples_per_s_call": nsamp / (statistics.median(wall) * 1e-3)}
            print("T %3d D %2d %-11s kernel %8.3f ms (%.3f .. %.3f), call %8.3f ms: %.3g input samples per s"
                  % (T, D, name, m, min(ms), max(ms), leg["call_ms"], leg["input_samples_per_s"]), flush=True)
            out["legs"].append(leg)
    b.close()

print(json.dumps(out))
dst_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "fr01_fir_rate.json")
with open(dst_path, "w") as f:
    json.dump(out, f, indent=1)
