"""What tracking costs: gpsbb_device_track on one resident render of six satellites, 0.1 s at 2.6 MS/s and at 25 MS/s, with 6, 12 and
32 channels (the six acquisition hits, repeated: two channels may carry one PRN) in SC16 / SC8 / SC1 — milliseconds per call (the
kernel by HIP events: the experiments build's gpsbb_test_track_ms; the whole synchronous call by the host's clock) and samples x
channels correlated per second.  One workgroup per channel: the figures say what one CU does with a channel, not what the part
could do.  No threshold: the figures go on record.

    GPSBB_PY_LIB=exp python tools/track_rate.py [--json OUT] [--quick]     (env: REPEATS=5)
Default output: profiles/tk01_track_rate.json.
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
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()

repeats = int(os.environ.get("REPEATS", "5"))
quick = "--quick" in sys.argv
L = pkg.lib()
if not hasattr(L, "gpsbb_test_track_ms"):
    sys.exit("the experiments build is wanted (GPSBB_PY_LIB=exp): the kernel's time comes from its hook")
L.gpsbb_test_track_ms.argtypes = [C.c_void_p]
L.gpsbb_test_track_ms.restype = C.c_float

out = {"tool": "track_rate", "repeats": repeats, "quick": quick, "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"], "shapes": []}
with pkg.Synth(0) as s:
    for fs in (2.6e6, 25e6):
        delt = 1.0 / fs
        nsamp = int(round(fs * 0.1))
        ch = pkg.synth_descriptors(1, nch=6, seed=0xACC)
        b = s.batch(ch, delt, nsamp)
        b.run()
        s.sync()
        trk = pkg.trk_make(delt, max_epochs=128)
        shape = {"fs": fs, "nsamp": nsamp, "legs": []}
        for name, fmt in (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(3)), ("sc1", pkg.OUT_SC1)):
            acq = pkg.acq_make(delt, -5000.0, 250.0, 41, 1e-3, 0, 2, fmt)
            rows = s.device_acquire(b.device_iq(), acq.nnc * acq.ncoh + acq.nlags - 1, acq, fmt)
            six = np.zeros(6, pkg.TRK_STATE_DTYPE)
            for k in range(6):
                kb, lag, _, _ = pkg.acq_best(rows, acq, k + 1)
                six[k] = pkg.trk_seed(acq, k + 1, kb, lag)
            for nch in (6, 12, 32):
                st = np.resize(six, nch)
                _, recs = s.device_track(b.device_iq(), nsamp, trk, st, fmt)   # warm: the scratch
                work = float(sum(int(r["N"].sum()) for r in recs))
                ms, wall = [], []
                for _ in range(1 if quick else repeats):
                    t0 = time.perf_counter()
                    s.device_track(b.device_iq(), nsamp, trk, st, fmt)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(float(L.gpsbb_test_track_ms(s._h)))
                m = statistics.median(ms)
                leg = {"view": name, "channels": nch, "epochs_per_channel": int(recs[0].size), "kernel_ms": m, "kernel_ms_min": min(ms),
                       "kernel_ms_max": max(ms), "call_ms": statistics.median(wall), "channel_samples": work,
                       "channel_samples_per_s": work / (m * 1e-3)}
                print("%5.1f MS/s %-5s %2d channels %9.3f ms (%.3f .. %.3f), call %9.3f ms: %.3g samples x channels per s"
                      % (fs / 1e6, name, nch, m, min(ms), max(ms), leg["call_ms"], leg["channel_samples_per_s"]), flush=True)
                shape["legs"].append(leg)
        b.close()
        out["shapes"].append(shape)

print(json.dumps(out))
dst = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "tk01_track_rate.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
