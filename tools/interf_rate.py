"""Interference (include/gpsbb.h gpsbb_interf_t) on the host-bound outputs: the chained host-gather stream at 16 ch / 25 MS/s with
32-block slots (tools/noise_rate.py's workload), in ONE process alternating four legs for each format (SC16, SC8, SC1): noise only,
noise only again (the A/A pair: its spread is the margin the other ratios are read against), noise + 1 emitter, noise + 4
emitters; then gpsbb_device_impair in place on a device buffer beside gpsbb_device_noise.  Reports IQ samples/s (median of
REPEATS timed runs of NSL slots, per leg).

    python tools/interf_rate.py [--json OUT] [--device-only [N]]   (env: GB=32 DEPTH=5 NSL=24 REPEATS=3 SHIFT=5 CN0=45 NSHIFT=1)
--device-only times the device calls alone, with N emitters (default 4; 0: gpsbb_device_noise): the run to put under rocprofv3
for the kernels' counters.
"""
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
import bench  # noqa: E402

gb = int(os.environ.get("GB", "32"))
depth = int(os.environ.get("DEPTH", "5"))
nsl = int(os.environ.get("NSL", "24"))
repeats = int(os.environ.get("REPEATS", "3"))
shift = int(os.environ.get("SHIFT", "5"))
cn0 = float(os.environ.get("CN0", "45"))
nshift = int(os.environ.get("NSHIFT", "1"))
nsamp, fs = 2500000, 25e6
delt = 1 / fs
sigma = pkg.noise_sigma(cn0, 1.0, delt)
NZ = pkg.Noise(1, 0, sigma, nshift, 0)
# a pulsed full-band chirp, a tone, a pulsed tone, a narrow chirp: every branch of the per-emitter arithmetic
EM = [pkg.interf_make(pkg.INTERF_CHIRP, 10.0, -fs / 2, fs / 2, 1e-4, 1e-3, 0.5, delt=delt),
      pkg.interf_make(pkg.INTERF_CW, 0.0, 1.0e6, delt=delt),
      pkg.interf_make(pkg.INTERF_CW, 6.0, -3.3e6, pulse_period_s=2e-4, duty=0.25, delt=delt),
      pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -2e6, 2e6, 3.01e-5, delt=delt)]
SETS = {1: pkg.InterfSet(EM[:1], nshift, 0), 4: pkg.InterfSet(EM, nshift, 0)}

out = {"tool": "interf_rate", "fs": fs, "nch": 16, "nsamp": nsamp, "blocks_per_slot": gb, "depth": depth, "slots": nsl,
       "repeats": repeats, "sc8_shift": shift, "cn0_dbhz": cn0, "sigma": sigma, "shift": nshift, "stream": [], "device": {}}

device_only = "--device-only" in sys.argv
dev_n = 4
if device_only and len(sys.argv) > sys.argv.index("--device-only") + 1 and sys.argv[sys.argv.index("--device-only") + 1].isdigit():
    dev_n = int(sys.argv[sys.argv.index("--device-only") + 1])
LEGS = (("noise", None), ("noise_again", None), ("noise+1", SETS[1]), ("noise+4", SETS[4]))

with pkg.Synth(0) as s:
    ch = None if device_only else bench.stream_descriptors(pkg, gb * 16, 16)
    for name, fmt in () if device_only else (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(shift)), ("sc1", pkg.OUT_SC1)):
        legs = {}
        for leg, js in LEGS:
            st = s.stream(16, delt, nsamp, gb, depth=depth, flags=pkg.CHAIN_CARRIER, fmt=fmt, noise=NZ, interf=js)
            legs[leg] = (st, {"pushed": 0})

        def run(st, state, n):
            pushed = popped = 0
            while popped < n:
                while pushed < n and st.pending < depth:
                    k = state["pushed"] % 16
                    st.push(ch[k * gb:(k + 1) * gb])
                    state["pushed"] += 1
                    pushed += 1
                st.pop(copy=False)
                popped += 1

        for st, state in legs.values():
            run(st, state, depth)  # warm-up: every slot's tables and buffers in place
        secs = {leg: [] for leg, _ in LEGS}
        for _ in range(repeats):
            for leg, _ in LEGS:
                st, state = legs[leg]
                t0 = time.perf_counter()
                run(st, state, nsl)
                secs[leg].append(time.perf_counter() - t0)
        for st, _ in legs.values():
            st.close()
        samples = nsl * gb * nsamp
        r = {"format": name, "flags": fmt}
        for leg, _ in LEGS:
            dt = statistics.median(secs[leg])
            r[leg] = {"samples_per_s": samples / dt, "ms_per_slot": dt / nsl * 1e3, "min_s": min(secs[leg]), "max_s": max(secs[leg])}
        base = r["noise"]["samples_per_s"]
        r["aa_spread"] = r["noise_again"]["samples_per_s"] / base
        r["plus1_vs_noise"] = r["noise+1"]["samples_per_s"] / base
        r["plus4_vs_noise"] = r["noise+4"]["samples_per_s"] / base
        out["stream"].append(r)
        print("%-4s noise %.3e samples/s  A/A x%.3f  +1 emitter x%.3f  +4 emitters x%.3f" % (
            name, base, r["aa_spread"], r["plus1_vs_noise"], r["plus4_vs_noise"]), flush=True)

    # the device calls in place: one slot's worth of int16 IQ in HBM
    n_dev = gb * nsamp
    d = torch.zeros(n_dev * 2, dtype=torch.int16, device="cuda")
    for label, js in ((("noise", None), ("noise+1", SETS[1]), ("noise+4", SETS[4]), ("4 alone", SETS[4])) if not device_only else
                      (("noise+%d" % dev_n, pkg.InterfSet(EM[:dev_n], nshift, 0) if dev_n else None),)):
        nz = None if label.endswith("alone") else NZ
        s.device_impair(d.data_ptr(), gb, nsamp, nz, js)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            s.device_impair(d.data_ptr(), gb, nsamp, nz, js)
            t.append(time.perf_counter() - t0)
        dt = statistics.median(t)
        out["device"][label] = {"samples": n_dev, "ms": dt * 1e3, "samples_per_s": n_dev / dt}
        print("device %-8s %.3e samples/s (%.2f ms for %d samples)" % (label, n_dev / dt, dt * 1e3, n_dev), flush=True)
    out["device"]["note"] = "synchronous calls, in place, int16 to int16; wall time includes the launch and the wait"
    del d

print(json.dumps(out))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f, indent=1)
