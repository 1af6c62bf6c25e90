"""Receiver noise (include/gpsbb.h gpsbb_noise_t) on the host-bound outputs: the chained host-gather stream at 16 ch / 25 MS/s with
32-block slots (tools/format_rate.py's workload), noise off and on alternating in one process for each format (SC16, SC8, SC1);
gpsbb_device_noise in place on a device buffer; and the drop-in fill at the reference geometry (12 ch, 2.6 MS/s, 300 000 samples,
registered iq_buff) with and without noise.  Reports IQ samples/s (median of REPEATS timed runs of NSL slots, per leg).

    python tools/noise_rate.py [--json OUT] [--device-only]   (env: GB=32 DEPTH=5 NSL=24 REPEATS=3 SHIFT=5 CN0=45 NSHIFT=1 FILLS=200)
--device-only times gpsbb_device_noise alone (the run to put under rocprofv3 for the noise kernel's counters).
GPSBB_PY_LIB=<experiments build> with GPSBB_NOISE_WGS=<n> sizes the noise kernel's grid (the product's is fixed).
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
fills = int(os.environ.get("FILLS", "200"))
nsamp, fs = 2500000, 25e6
ch = bench.stream_descriptors(pkg, gb * 16, 16)
sigma = pkg.noise_sigma(cn0, 1.0, 1 / fs)
NZ = {"seed": 1, "sample0": 0, "sigma": sigma, "shift": nshift}

out = {"tool": "noise_rate", "fs": fs, "nch": 16, "nsamp": nsamp, "blocks_per_slot": gb, "depth": depth, "slots": nsl,
       "repeats": repeats, "sc8_shift": shift, "cn0_dbhz": cn0, "sigma": sigma, "noise_shift": nshift,
       "noise_wgs": os.environ.get("GPSBB_NOISE_WGS", "product"), "stream": [], "device_noise": {}, "fill": {}}

device_only = "--device-only" in sys.argv
with pkg.Synth(0) as s:
    for name, fmt in () if device_only else (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(shift)), ("sc1", pkg.OUT_SC1)):
        legs = {}
        for noise in (None, NZ):
            st = s.stream(16, 1 / fs, nsamp, gb, depth=depth, flags=pkg.CHAIN_CARRIER, fmt=fmt, noise=noise)
            legs["on" if noise else "off"] = (st, {"pushed": 0})

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
        secs = {"off": [], "on": []}
        for _ in range(repeats):
            for leg in ("off", "on"):
                st, state = legs[leg]
                t0 = time.perf_counter()
                run(st, state, nsl)
                secs[leg].append(time.perf_counter() - t0)
        for st, _ in legs.values():
            st.close()
        samples = nsl * gb * nsamp
        r = {"format": name, "flags": fmt}
        for leg in ("off", "on"):
            dt = statistics.median(secs[leg])
            r[leg] = {"samples_per_s": samples / dt, "ms_per_slot": dt / nsl * 1e3, "min_s": min(secs[leg]), "max_s": max(secs[leg])}
        r["on_vs_off"] = r["on"]["samples_per_s"] / r["off"]["samples_per_s"]
        out["stream"].append(r)
        print("%-4s off %.3e  on %.3e samples/s  (x%.3f)" % (name, r["off"]["samples_per_s"], r["on"]["samples_per_s"], r["on_vs_off"]),
              flush=True)
    if not device_only:
        out["noise_clipped_components"] = s.info(pkg.INFO_NOISE_CLIPPED)

    # gpsbb_device_noise in place: one slot's worth of int16 IQ in HBM
    n_dev = gb * nsamp
    d = torch.zeros(n_dev * 2, dtype=torch.int16, device="cuda")
    s.device_noise(d.data_ptr(), gb, nsamp, NZ)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        s.device_noise(d.data_ptr(), gb, nsamp, NZ)
        t.append(time.perf_counter() - t0)
    dt = statistics.median(t)
    out["device_noise"] = {"samples": n_dev, "ms": dt * 1e3, "samples_per_s": n_dev / dt,
                           "note": "synchronous call, in place, int16 to int16; wall time includes the launch and the wait"}
    print("device_noise %.3e samples/s (%.2f ms for %d samples)" % (n_dev / dt, dt * 1e3, n_dev), flush=True)
    del d

    # the drop-in fill at the reference geometry, registered iq_buff
    import numpy as np
    if device_only:
        fills = 0
    fch = pkg.synth_descriptors(max(fills, 1), nch=12, seed=0x5EED)
    f_nsamp, f_fs = 300000, 2.6e6
    buf = np.zeros(f_nsamp * 4, np.uint8)
    s.host_register(buf)
    nzf = {"seed": 1, "sample0": 0, "sigma": pkg.noise_sigma(cn0, 1.0, 1 / f_fs), "shift": 0}
    lat = {"off": [], "on": []}
    for k in range(fills):
        for leg in ("off", "on"):
            t0 = time.perf_counter()
            s.fill_block(fch[k], 1 / f_fs, f_nsamp, out=buf.view(np.int16).reshape(f_nsamp, 2),
                         noise=dict(nzf, sample0=k * f_nsamp) if leg == "on" else None)
            lat[leg].append((time.perf_counter() - t0) * 1e3)
    s.host_unregister(buf)
    for leg in ("off", "on") if fills > 2 else ():
        v = sorted(lat[leg][2:])
        out["fill"][leg] = {"p50_ms": v[len(v) // 2], "p99_ms": v[int(len(v) * 0.99)], "max_ms": v[-1]}
    out["fill"]["geometry"] = {"nch": 12, "fs": f_fs, "nsamp": f_nsamp, "registered": True, "calls": fills}
    if fills > 2:
        print("fill 12 ch 2.6 MS/s 300000: off p50 %.3f ms, on p50 %.3f ms" % (out["fill"]["off"]["p50_ms"], out["fill"]["on"]["p50_ms"]),
              flush=True)

print(json.dumps(out))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f, indent=1)
