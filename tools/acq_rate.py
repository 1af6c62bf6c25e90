"""What the blind search costs: gpsbb_device_acquire on one resident render at 2.6 MS/s (N = P = 2600) and one at 25 MS/s
(N = P = 25000), 21 bins, 32 PRNs, two intervals, in SC16 / SC8 / SC1 — milliseconds per call (the three kernels, by HIP events:
the experiments build's gpsbb_test_acquire_ms; and the whole synchronous call by the host's clock) and cells searched per second
(PRN x bin x delay x sample), beside k_despread_lags' (channel x lag x sample) per second on the same batch in the same run, and
the share of the i8 MFMA rate the digit planes' products reach.  No threshold: the figures go on record.

    GPSBB_PY_LIB=exp python tools/acq_rate.py [--json OUT] [--quick]     (env: REPEATS=5)
Default output: profiles/aq01_acq_rate.json.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
os.environ.setdefault("GPSBB_PY_LIB", "exp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()

# dense i8 MFMA: twice the BF16 form's K in the BF16 form's cycles, and BF16 dense is about 2.5e15 FLOP/s on this part
I8_PEAK_OPS = 5.0e15
DIGITS = {"sc16": 4, "sc8": 3, "sc1": 2}

repeats = int(os.environ.get("REPEATS", "5"))
quick = "--quick" in sys.argv
L = pkg.lib()
if not hasattr(L, "gpsbb_test_acquire_ms"):
    sys.exit("the experiments build is wanted (GPSBB_PY_LIB=exp): the kernels' time comes from its hook")
L.gpsbb_test_acquire_ms.argtypes = [C.c_void_p]
L.gpsbb_test_acquire_ms.restype = C.c_float
L.gpsbb_test_despread_ms.argtypes = [C.c_void_p]
L.gpsbb_test_despread_ms.restype = C.c_float

LAGS = (-3, -2, -1, 0, 1, 2, 3, 4)
out = {"tool": "acq_rate", "repeats": repeats, "quick": quick, "i8_peak_ops_per_s": I8_PEAK_OPS,
       "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"], "shapes": []}
with pkg.Synth(0) as s:
    for fs in (2.6e6, 25e6):
        delt = 1.0 / fs
        views = (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(3)), ("sc1", pkg.OUT_SC1))
        cfgs = {name: pkg.acq_make(delt, -5000.0, 500.0, 21, 1e-3, 0, 2, fmt) for name, fmt in views}
        c0 = cfgs["sc16"]
        nsamp = c0.nnc * c0.ncoh + c0.nlags - 1
        ch = pkg.synth_descriptors(1, nch=16, seed=0xACC)
        b = s.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
        b.run()
        s.sync()
        shape = {"fs": fs, "nsamp": nsamp, "ncoh": c0.ncoh, "nlags": c0.nlags, "nnc": c0.nnc, "nbins": c0.nbins, "prns": 32,
                 "variant": s.info(pkg.INFO_LAST_VARIANT), "legs": []}
        legs = [(name, (lambda n, f: lambda: s.device_acquire(b.device_iq(), nsamp, cfgs[n], f))(name, fmt)) for name, fmt in views]
        legs.append(("despread_lags8", lambda: b.despread_lags(LAGS, seg_tiles=1)))
        for k, f in list(legs):   # warm: the scratch
            try:
                f()
            except pkg.GpsbbError as e:   # (a batch the per-sample kernel took has no tile states to despread with)
                print("%s not measured at %.1f MS/s: %s" % (k, fs / 1e6, e), flush=True)
                legs = [x for x in legs if x[0] != k]
        ms = {k: [] for k, _ in legs}
        wall = {k: [] for k, _ in legs}
        for r in range(1 if quick else repeats):
            for k, f in (legs if r % 2 == 0 else legs[::-1]):
                t0 = time.perf_counter()
                f()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                ms[k].append(float(L.gpsbb_test_despread_ms(b._b) if k == "despread_lags8" else L.gpsbb_test_acquire_ms(s._h)))
        for k, t in ms.items():
            m = statistics.median(t)
            leg = {"leg": k, "kernel_ms": m, "kernel_ms_min": min(t), "kernel_ms_max": max(t), "call_ms": statistics.median(wall[k])}
            if k == "despread_lags8":
                leg["channel_lag_samples_per_s"] = 16 * len(LAGS) * nsamp / (m * 1e-3)
                print("%5.1f MS/s %-14s %9.3f ms (%.3f .. %.3f), call %9.3f ms: %.3g channel x lag x sample per s"
                      % (fs / 1e6, k, m, min(t), max(t), leg["call_ms"], leg["channel_lag_samples_per_s"]), flush=True)
            else:
                c = cfgs[k]
                cells = 32.0 * c.nbins * c.nlags * c.nnc * c.ncoh
                ntiles, npad = -(-c.nlags // 32), -(-c.ncoh // 32) * 32
                mfma_ops = 2.0 * 32 * (ntiles * 32) * npad * c.nnc * c.nbins * 2 * DIGITS[k]
                leg.update(cells_per_s=cells / (m * 1e-3), digit_planes=2 * DIGITS[k], mfma_ops=mfma_ops,
                           share_of_i8_peak=mfma_ops / (m * 1e-3) / I8_PEAK_OPS)
                print("%5.1f MS/s %-14s %9.3f ms (%.3f .. %.3f), call %9.3f ms: %.3g PRN x bin x delay x sample per s, %.1f %% of the i8 MFMA rate"
                      % (fs / 1e6, k, m, min(t), max(t), leg["call_ms"], leg["cells_per_s"], 100.0 * leg["share_of_i8_peak"]), flush=True)
            shape["legs"].append(leg)
        b.close()
        out["shapes"].append(shape)

print(json.dumps(out))
dst = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "aq01_acq_rate.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
