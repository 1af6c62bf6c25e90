"""What the blanker costs: gpsbb_device_blank (L = G = hold = 8, a threshold nothing passes) over 25 000 000 resident int16 IQ
samples, plain, with noise, and with noise and a chirp — milliseconds per call (the kernels by HIP events: the experiments build's
gpsbb_test_blank_ms; the whole synchronous call by the host's clock), the median of five, samples per second, and the kernel's share
of the HBM floor of 8 bytes per sample (4 read, 4 written) at HBM_BYTES_PER_S.

The yardstick is gpsbb_device_fir with T = 1, D = 1 (the identity filter: the same view, the same 8 bytes per sample) on the same
buffers in the same process, the two alternating call by call: fir, blank, fir, blank, ...  Beside the ratio blank / fir stands an
A/A pair, the fir's odd runs against its even runs, whose spread is the margin the ratio is read against.  A second plan at the
ranges' end (L = 64, G = 255, hold = 1023) shows what the longest halo costs.  No threshold on the figures: they go on record.

    GPSBB_PY_LIB=exp python tools/blank_rate.py [--json OUT] [--quick]     (env: REPEATS=5)
Default output: profiles/bl01_blank_rate.json.
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
import fir_check as fc  # noqa: E402

pkg = load_package()

repeats = int(os.environ.get("REPEATS", "5"))
quick = "--quick" in sys.argv
L = pkg.lib()
if not hasattr(L, "gpsbb_test_blank_ms"):
    sys.exit("the experiments build is wanted (GPSBB_PY_LIB=exp): the kernels' time comes from its hook")
for fn in (L.gpsbb_test_blank_ms, L.gpsbb_test_fir_ms):
    fn.argtypes = [pkg.C.c_void_p]
    fn.restype = pkg.C.c_float

HBM_BYTES_PER_S = 8.0e12   # MI355X: 8 TB/s peak
noise = {"seed": 0xB5D, "sample0": (1 << 32) + 12345, "sigma": 700.0, "shift": 1}
NSAMP = 2500000 if quick else 25000000
NEVER = (1 << 64) - 1


def alternating(calls, rounds):
    """calls: name -> (call, hook); every round runs each once, in order -> name -> ([kernel ms], [call ms])"""
    for call, _ in calls.values():
        call()   # warm: the scratch, the noise table
    got = {k: ([], []) for k in calls}
    for _ in range(rounds):
        for k, (call, hook) in calls.items():
            t0 = time.perf_counter()
            call()
            got[k][1].append((time.perf_counter() - t0) * 1e3)
            got[k][0].append(float(hook()))
    return got


out = {"tool": "blank_rate", "repeats": repeats, "quick": quick, "nsamp": NSAMP, "hbm_bytes_per_s": HBM_BYTES_PER_S,
       "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "legs": []}
floor_ms = NSAMP * 8 / HBM_BYTES_PER_S * 1e3
with pkg.Synth(0) as s:
    src = torch.randint(-8000, 8000, (NSAMP, 2), dtype=torch.int16, device="cuda")
    dst = torch.zeros((NSAMP, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ident = pkg.Fir([1], 1, 0)
    for shape in ((8, 8, 8), (64, 255, 1023)):
        b = pkg.Blank(shape[0], shape[1], shape[2], NEVER)
        for name, nz, js in (("plain", None, None), ("noise", noise, None), ("noise + chirp", noise, fc.chirp_set(pkg))):
            if js is not None:
                js = pkg.InterfSet([js.e[k] for k in range(js.n)], noise["shift"], noise["sample0"])
            rounds = 1 if quick else 2 * repeats
            got = alternating({"fir": (lambda: s.device_fir(src.data_ptr(), NSAMP, ident, dst.data_ptr(), None, nz, js), lambda: L.gpsbb_test_fir_ms(s._h)),
                               "blank": (lambda: s.device_blank(src.data_ptr(), NSAMP, b, dst.data_ptr(), None, nz, js), lambda: L.gpsbb_test_blank_ms(s._h)),
                               "blank_nt": (lambda: (L.gpsbb_test_blank_nt(1), s.device_blank(src.data_ptr(), NSAMP, b, dst.data_ptr(), None, nz, js),
                                                     L.gpsbb_test_blank_nt(0)), lambda: L.gpsbb_test_blank_ms(s._h))},
                              rounds)
            fir_ms, blank_ms, nt_ms = got["fir"][0], got["blank"][0], got["blank_nt"][0]
            m, fm = statistics.median(blank_ms), statistics.median(fir_ms)
            aa = statistics.median(fir_ms[0::2]) / statistics.median(fir_ms[1::2]) if len(fir_ms) > 1 else float("nan")
            leg = {"plan": list(shape), "view": name, "kernel_ms": m, "kernel_ms_min": min(blank_ms), "kernel_ms_max": max(blank_ms),
                   "call_ms": statistics.median(got["blank"][1]), "samples_per_s": NSAMP / (m * 1e-3), "hbm_floor_ms": floor_ms, "share_of_hbm_floor": floor_ms / m,
                   "fir_identity_kernel_ms": fm, "fir_identity_kernel_ms_min": min(fir_ms), "fir_identity_kernel_ms_max": max(fir_ms),
                   "fir_identity_call_ms": statistics.median(got["fir"][1]), "blank_over_fir": m / fm, "fir_aa_odd_over_even": aa,
                   "blank_kernel_ms_all": blank_ms, "fir_kernel_ms_all": fir_ms, "nontemporal_stores_kernel_ms": statistics.median(nt_ms),
                   "nontemporal_stores_kernel_ms_all": nt_ms, "nontemporal_over_plain": statistics.median(nt_ms) / m}
            print("blank %r %-13s kernels %7.3f ms (%.3f .. %.3f), call %7.3f ms: %.3g samples per s, %.1f %% of the floor; identity fir %7.3f ms "
                  "(%.3f .. %.3f): blank / fir %.3f, the fir's A/A %.3f; with non-temporal stores %7.3f ms"
                  % (shape, name, m, min(blank_ms), max(blank_ms), leg["call_ms"], leg["samples_per_s"], 100 * leg["share_of_hbm_floor"], fm, min(fir_ms),
                     max(fir_ms), m / fm, aa, leg["nontemporal_stores_kernel_ms"]), flush=True)
            out["legs"].append(leg)

print(json.dumps({k: v for k, v in out.items() if k != "legs"}))
dst_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "bl01_blank_rate.json")
with open(dst_path, "w") as f:
    json.dump(out, f, indent=1)
