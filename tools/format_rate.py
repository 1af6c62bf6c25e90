"""The host-bound output formats (include/gpsbb.h GPSBB_OUT_*) through a chained host-gather stream at 16 ch / 25 MS/s, one format
after the other in one process: SC16 (int16, today's gather), SC8 (int8: half the bytes) and SC1 (1-bit packed: a sixteenth).
Reports IQ samples/s and GB/s reaching host memory for each (median of REPEATS timed runs of NSL slots of GB blocks).

    python tools/format_rate.py [--json OUT]        (env: GB=32 DEPTH=5 NSL=48 REPEATS=3 SHIFT=5)
"""
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
import bench  # noqa: E402

gb = int(os.environ.get("GB", "32"))
depth = int(os.environ.get("DEPTH", "5"))
nsl = int(os.environ.get("NSL", "48"))
repeats = int(os.environ.get("REPEATS", "3"))
shift = int(os.environ.get("SHIFT", "5"))
nsamp, fs = 2500000, 25e6
ch = bench.stream_descriptors(pkg, gb * 16, 16)

results = []
with pkg.Synth(0) as s:
    for name, fmt in (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(shift)), ("sc1", pkg.OUT_SC1)):
        st = s.stream(16, 1 / fs, nsamp, gb, depth=depth, flags=pkg.CHAIN_CARRIER, fmt=fmt)
        state = {"pushed": 0}

        def run(n):
            pushed = popped = 0
            while popped < n:
                while pushed < n and st.pending < depth:
                    k = state["pushed"] % 16
                    st.push(ch[k * gb:(k + 1) * gb])
                    state["pushed"] += 1
                    pushed += 1
                st.pop(copy=False)
                popped += 1

        run(depth)  # warm-up: every slot's tables and buffers in place
        secs = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            run(nsl)
            secs.append(time.perf_counter() - t0)
        st.close()
        dt = statistics.median(secs)
        samples = nsl * gb * nsamp
        r = {"format": name, "flags": fmt, "blocks_per_slot": gb, "depth": depth, "slots": nsl, "repeats": repeats,
             "samples_per_s": samples / dt, "gb_per_s_to_host": samples * pkg.out_bytes(fmt, nsamp) / nsamp / dt / 1e9,
             "ms_per_slot": dt / nsl * 1e3, "min_s": min(secs), "max_s": max(secs)}
        if name == "sc8":
            r["clipped_components"] = s.info(pkg.INFO_SC8_CLIPPED)
        results.append(r)
        print("%-4s %.3e samples/s  %6.1f GB/s to host  %.2f ms per slot of %d blocks" %
              (name, r["samples_per_s"], r["gb_per_s_to_host"], r["ms_per_slot"], gb), flush=True)

base = results[0]["samples_per_s"]
for r in results:
    r["x_sc16"] = r["samples_per_s"] / base
print(json.dumps({"tool": "format_rate", "fs": fs, "nch": 16, "nsamp": nsamp, "shift": shift, "results": results}))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump({"tool": "format_rate", "fs": fs, "nch": 16, "nsamp": nsamp, "shift": shift, "results": results}, f, indent=1)
