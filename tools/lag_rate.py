"""What the lags cost beside the prompt sum: gpsbb_batch_despread_lags at 1, 3 and 8 lags against gpsbb_batch_despread_impaired
on one resident batch, in one process, warm, the legs alternating within every round; the prompt call runs twice per round (the
A/A pair: its spread is the margin the ratios are read against).  Kernel times by HIP events (the experiments build's
gpsbb_test_despread_ms).  Expected from instruction counts: (37 + 3 * nlags) / 37 of the prompt call per
channel-sample, and 2/16 more view work where a lag looks to either side.

    GPSBB_PY_LIB=exp python tools/lag_rate.py [--json OUT] [--quick]     (env: REPEATS=5 SEG_TILES=16 CN0=45)
Default output: profiles/mp01_lag_rate.json.
"""
import ctypes as C
import json
import os
import statistics
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
os.environ.setdefault("GPSBB_PY_LIB", "exp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime for torch and libgpsbb: imported first, as the tests do)

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
import bench  # noqa: E402

repeats = int(os.environ.get("REPEATS", "5"))
seg_tiles = int(os.environ.get("SEG_TILES", "16"))
cn0 = float(os.environ.get("CN0", "45"))
quick = "--quick" in sys.argv
L = pkg.lib()
if not hasattr(L, "gpsbb_test_despread_ms"):
    sys.exit("the experiments build is wanted (GPSBB_PY_LIB=exp): the kernel's time comes from its hook")
L.gpsbb_test_despread_ms.argtypes = [C.c_void_p]
L.gpsbb_test_despread_ms.restype = C.c_float

LAG_SETS = {"lags1": (0,), "lags3": (-1, 0, 1), "lags8": (-3, -2, -1, 0, 1, 2, 3, 4)}
out = {"tool": "lag_rate", "repeats": repeats, "seg_tiles": seg_tiles, "cn0_dbhz": cn0, "quick": quick,
       "lag_sets": {k: list(v) for k, v in LAG_SETS.items()}, "shapes": []}
with pkg.Synth(0) as s:
    for name, fs, nch, nsamp, nblocks, nshift in (("headline", 25e6, 16, 2500000, 100, 1), ("reference", 2.6e6, 12, 300000, 400, 0)):
        if quick:
            nblocks //= 10
        delt = 1.0 / fs
        ch = bench.stream_descriptors(pkg, nblocks, nch)
        b = s.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
        b.run()
        s.sync()
        variant = s.info(pkg.INFO_LAST_VARIANT)
        nz = pkg.Noise(1, 0, pkg.noise_sigma(cn0, 1.0, delt), nshift, 0)
        shape = {"name": name, "fs": fs, "nch": nch, "nsamp": nsamp, "nblocks": nblocks, "samples": nblocks * nsamp, "variant": variant, "legs": []}
        for noise in (None, nz):
            def prompt():
                b.despread(noise=noise, seg_tiles=seg_tiles)   # (gpsbb_batch_despread_impaired with no set)

            legs = [("prompt_a", prompt), ("prompt_b", prompt)] + [
                (k, (lambda v: lambda: b.despread_lags(v, seg_tiles=seg_tiles, noise=noise))(v)) for k, v in LAG_SETS.items()]
            for _, f in legs:   # warm: the scratch, the noise table
                f()
            ms = {k: [] for k, _ in legs}
            for r in range(repeats):
                for k, f in (legs if r % 2 == 0 else legs[::-1]):
                    f()
                    ms[k].append(float(L.gpsbb_test_despread_ms(b._b)))
            base = statistics.median(ms["prompt_a"])
            for k, t in ms.items():
                m = statistics.median(t)
                nl = len(LAG_SETS[k]) if k in LAG_SETS else 0
                expect = None if not nl else (37.0 + 3.0 * nl) / 37.0
                shape["legs"].append({"leg": k, "noise": noise is not None, "ms": m, "ms_min": min(t), "ms_max": max(t), "vs_prompt_a": m / base,
                                      "expected_vs_prompt_per_channel_sample": expect})
                print("%-9s noise %-5s %-9s %8.3f ms (%.3f .. %.3f)  x%.3f of the prompt call%s"
                      % (name, noise is not None, k, m, min(t), max(t), m / base, "" if expect is None else "  (replica arithmetic alone: x%.3f)" % expect),
                      flush=True)
        b.close()
        out["shapes"].append(shape)

print(json.dumps(out))
dst = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "mp01_lag_rate.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
