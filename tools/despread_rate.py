"""What looking at a block costs beside rendering it: gpsbb_batch_despread on a resident batch, in one process, warm, alternating
with the batch's own re-run — the shapes of bench.py's headline (16 ch, 25 MS/s, 400 blocks of 2 500 000 samples) and of the
reference's geometry (12 ch, 2.6 MS/s, 1000 blocks of 300 000).  Per view (SC16 / SC8 / SC1, with and without fused noise): the
kernel's time by HIP events (the experiments build's gpsbb_test_despread_ms), samples/s and bytes read over time; beside it
ms_synth of the same batch's run (gpsbb_batch_last_timing): the synthesis kernel is not touched by despreading, so the ratio is
against the code as it was.

    GPSBB_PY_LIB=exp python tools/despread_rate.py [--json OUT] [--quick]     (env: REPEATS=5 SEG_TILES=16 CN0=45)
--quick: a tenth of the blocks (a smoke of the tool, or the run to put under rocprofv3 --kernel-trace --stats).
"""
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
import ctypes as C  # noqa: E402
L.gpsbb_test_despread_ms.argtypes = [C.c_void_p]
L.gpsbb_test_despread_ms.restype = C.c_float

out = {"tool": "despread_rate", "repeats": repeats, "seg_tiles": seg_tiles, "cn0_dbhz": cn0, "quick": quick, "shapes": []}
with pkg.Synth(0) as s:
    for name, fs, nch, nsamp, nblocks, nshift, shift8 in (("headline", 25e6, 16, 2500000, 400, 1, 7), ("reference", 2.6e6, 12, 300000, 1000, 0, 6)):
        if quick:
            nblocks //= 10
        delt = 1.0 / fs
        ch = bench.stream_descriptors(pkg, nblocks, nch)
        b = s.batch(ch, delt, nsamp, flags=pkg.CHAIN_CARRIER)
        nz = pkg.Noise(1, 0, pkg.noise_sigma(cn0, 1.0, delt), nshift, 0)
        for _ in range(3):   # warm: every table set built, the output buffer in place
            b.run()
        s.sync()
        views = [("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(shift8)), ("sc1", pkg.OUT_SC1)]
        legs = [(v, f, n) for v, f in views for n in (None, nz)]
        for _, f, n in legs:
            b.despread(view=f, noise=n, seg_tiles=seg_tiles)   # warm: the scratch, the noise table
        ms = {(v, n is not None): [] for v, _, n in legs}
        synth_ms = []
        for _ in range(repeats):
            for v, f, n in legs:
                b.run()
                s.sync()
                synth_ms.append(b.timing()["ms_synth"])
                b.despread(view=f, noise=n, seg_tiles=seg_tiles)
                ms[(v, n is not None)].append(float(L.gpsbb_test_despread_ms(b._b)))
        variant = s.info(pkg.INFO_LAST_VARIANT)
        b.close()
        samples = nblocks * nsamp
        synth = statistics.median(synth_ms)
        shape = {"name": name, "fs": fs, "nch": nch, "nsamp": nsamp, "nblocks": nblocks, "samples": samples, "variant": variant,
                 "ms_synth": synth, "ms_synth_min": min(synth_ms), "ms_synth_max": max(synth_ms), "sc8_shift": shift8, "noise_shift": nshift,
                 "legs": []}
        for (v, noisy), t in ms.items():
            m = statistics.median(t)
            shape["legs"].append({"view": v, "noise": noisy, "ms": m, "ms_min": min(t), "ms_max": max(t), "samples_per_s": samples / (m * 1e-3),
                                  "read_GBps": 4.0 * samples / (m * 1e-3) / 1e9, "vs_synth": m / synth})
            print("%-9s %-4s noise %-5s %8.3f ms (%.3f .. %.3f)  %.3e samples/s  %.0f GB/s read  x%.2f of ms_synth %.3f"
                  % (name, v, noisy, m, min(t), max(t), samples / (m * 1e-3), 4.0 * samples / (m * 1e-3) / 1e9, m / synth, synth), flush=True)
        out["shapes"].append(shape)

print(json.dumps(out))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f, indent=1)
