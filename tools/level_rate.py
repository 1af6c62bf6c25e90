"""The output level (include/gpsbb.h gpsbb_level_t, k_level) beside the calls it shares a read side with, in ONE warm process:

(a) a resident 16 ch / 25 MS/s batch of 32 blocks: gpsbb_device_level's four variants (plain, noise, 4 emitters, both) alternating
    with gpsbb_device_noise and gpsbb_device_impair in place on the same buffer, the plain variant with gpsbb_device_digest; the
    in-place noise call and the plain level call run twice per round (the A/A pairs: their spread is the margin the ratios are
    read against);
(b) the chained host-gather ring of tools/noise_rate.py (32-block slots, noise at 45 dB-Hz) in SC16, SC8 and SC1: pushes without
    GPSBB_PUSH_LEVEL, the same again (A/A), pushes with it.

Medians of REPEATS rounds.  Writes profiles/lv01_level_rate.json.

    python tools/level_rate.py [--json OUT] [--device-only VARIANT]   (env: GB=32 DEPTH=5 NSL=24 REPEATS=5 SHIFT=5 CN0=45 NSHIFT=1)
--device-only plain|noise|set|both times that gpsbb_device_level variant alone: the run to put under rocprofv3.
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
nsl = int(os.environ.get("NSL", "24"))
repeats = int(os.environ.get("REPEATS", "5"))
shift = int(os.environ.get("SHIFT", "5"))
cn0 = float(os.environ.get("CN0", "45"))
nshift = int(os.environ.get("NSHIFT", "1"))
nsamp, fs = 2500000, 25e6
delt = 1 / fs
sigma = pkg.noise_sigma(cn0, 1.0, delt)
NZ = pkg.Noise(1, 0, sigma, nshift, 0)
# tools/interf_rate.py's four: a pulsed full-band chirp, a tone, a pulsed tone, a narrow chirp
EM = [pkg.interf_make(pkg.INTERF_CHIRP, 10.0, -fs / 2, fs / 2, 1e-4, 1e-3, 0.5, delt=delt),
      pkg.interf_make(pkg.INTERF_CW, 0.0, 1.0e6, delt=delt),
      pkg.interf_make(pkg.INTERF_CW, 6.0, -3.3e6, pulse_period_s=2e-4, duty=0.25, delt=delt),
      pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -2e6, 2e6, 3.01e-5, delt=delt)]
SET4 = pkg.InterfSet(EM, nshift, 0)

out = {"tool": "level_rate", "fs": fs, "nch": 16, "nsamp": nsamp, "blocks": gb, "depth": depth, "slots": nsl, "repeats": repeats,
       "sc8_shift": shift, "cn0_dbhz": cn0, "sigma": sigma, "shift": nshift, "device": {}, "stream": []}
only = sys.argv[sys.argv.index("--device-only") + 1] if "--device-only" in sys.argv else None

with pkg.Synth(0) as s:
    ch = bench.stream_descriptors(pkg, gb * 16, 16)
    # ---- (a) the resident batch ----
    b = s.batch(ch[:gb], delt, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    s.sync()
    d = b.device_iq()
    calls = {
        "level_plain": lambda: s.device_level(d, gb, nsamp),
        "digest": lambda: s.device_digest(d, gb, nsamp),
        "level_plain_again": lambda: s.device_level(d, gb, nsamp),
        "level_noise": lambda: s.device_level(d, gb, nsamp, NZ),
        "noise_in_place": lambda: s.device_noise(d, gb, nsamp, NZ),
        "noise_in_place_again": lambda: s.device_noise(d, gb, nsamp, NZ),
        "level_set": lambda: s.device_level(d, gb, nsamp, None, SET4),
        "impair_set_in_place": lambda: s.device_impair(d, gb, nsamp, None, SET4),
        "level_both": lambda: s.device_level(d, gb, nsamp, NZ, SET4),
        "impair_both_in_place": lambda: s.device_impair(d, gb, nsamp, NZ, SET4),
    }
    if only:
        calls = {"level_" + only: calls["level_" + only]}
    for f in calls.values():
        f()  # warm: code objects, the knot table, the result buffer
    secs = {k: [] for k in calls}
    for _ in range(repeats):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            secs[k].append(time.perf_counter() - t0)
    n_dev = gb * nsamp
    for k in calls:
        dt = statistics.median(secs[k])
        out["device"][k] = {"ms": dt * 1e3, "samples_per_s": n_dev / dt, "min_ms": min(secs[k]) * 1e3, "max_ms": max(secs[k]) * 1e3}
        print("device %-22s %.3e samples/s (%.3f ms for %d samples)" % (k, n_dev / dt, dt * 1e3, n_dev), flush=True)
    if not only:
        ms = {k: v["ms"] for k, v in out["device"].items()}
        out["device"]["ratios_time"] = {
            "aa_noise_in_place": ms["noise_in_place_again"] / ms["noise_in_place"],
            "aa_level_plain": ms["level_plain_again"] / ms["level_plain"],
            "level_noise_vs_noise_in_place": ms["level_noise"] / ms["noise_in_place"],
            "level_set_vs_impair_in_place": ms["level_set"] / ms["impair_set_in_place"],
            "level_both_vs_impair_in_place": ms["level_both"] / ms["impair_both_in_place"],
            "level_plain_vs_digest": ms["level_plain"] / ms["digest"],
        }
        for k, v in out["device"]["ratios_time"].items():
            print("  time ratio %-32s x%.3f" % (k, v), flush=True)
    out["device"]["note"] = "synchronous calls; wall time includes the launch, the wait and the result's copy; ratios are of times (above 1: slower)"
    lv = s.device_level(d, gb, nsamp, NZ, SET4)
    out["device"]["chosen_sc8_100ppm"] = list(pkg.level_choose(lv, pkg.OUT_SC8(0), 100.0))
    b.close()

    # ---- (b) the host-gather ring ----
    LEGS = (("plain", False), ("plain_again", False), ("level", True))
    for name, fmt in () if only else (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(shift)), ("sc1", pkg.OUT_SC1)):
        legs = {}
        for leg, flag in LEGS:
            st = s.stream(16, delt, nsamp, gb, depth=depth, flags=pkg.CHAIN_CARRIER, fmt=fmt, noise=NZ)
            legs[leg] = (st, {"pushed": 0}, flag)

        def run(st, state, flag, n):
            pushed = popped = 0
            while popped < n:
                while pushed < n and st.pending < depth:
                    k = state["pushed"] % 16
                    st.push(ch[k * gb:(k + 1) * gb], level=flag)
                    state["pushed"] += 1
                    pushed += 1
                if flag:
                    st.pop_level(copy=False)
                else:
                    st.pop(copy=False)
                popped += 1

        for st, state, flag in legs.values():
            run(st, state, flag, depth)  # warm-up: every slot's tables and buffers in place
        secs = {leg: [] for leg, _ in LEGS}
        for _ in range(repeats):
            for leg, _ in LEGS:
                st, state, flag = legs[leg]
                t0 = time.perf_counter()
                run(st, state, flag, nsl)
                secs[leg].append(time.perf_counter() - t0)
        for st, _, _ in legs.values():
            st.close()
        samples = nsl * gb * nsamp
        r = {"format": name, "flags": fmt}
        for leg, _ in LEGS:
            dt = statistics.median(secs[leg])
            r[leg] = {"samples_per_s": samples / dt, "ms_per_slot": dt / nsl * 1e3, "min_s": min(secs[leg]), "max_s": max(secs[leg])}
        base = r["plain"]["samples_per_s"]
        r["aa_spread"] = r["plain_again"]["samples_per_s"] / base
        r["level_vs_plain"] = r["level"]["samples_per_s"] / base
        out["stream"].append(r)
        print("%-4s plain %.3e samples/s  A/A x%.3f  with GPSBB_PUSH_LEVEL x%.3f" % (name, base, r["aa_spread"], r["level_vs_plain"]), flush=True)

print(json.dumps(out))
dest = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else (None if only else os.path.join(ROOT, "profiles", "lv01_level_rate.json"))
if dest:
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
