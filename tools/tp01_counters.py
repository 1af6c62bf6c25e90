#!/usr/bin/env python3
"""The exact-run and hazard counters of the cases of tests/test_ev_tile_prologue_gpu.py on the library GPSBB_PY_LIB names (the
parent commit's libgpsbb.so: what the test's PARENT table records), as one JSON line: name -> [exact runs, itable_512,
dwrd_oob, tiles rendered].
    GPSBB_PY_LIB=/path/to/parent/libgpsbb.so python tools/tp01_counters.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import test_ev_tile_prologue_gpu as t  # noqa: E402

pkg = conftest.load_package()
out = {"lib": pkg.LIB_PATH}
with pkg.Synth(0) as s:
    for name, make in t.CASES.items():
        ch, nsamp, flags = make(pkg)
        if name == "stream":
            for digest in (False, True):
                c0 = t.counters(pkg, s)
                q = s.stream(16, t.DELT, nsamp, 8, depth=3, flags=flags | pkg.STREAM_DEVICE_ONLY)
                for k in range(3):
                    q.push(ch[8 * k:8 * k + 8], digest=digest)
                s.sync()
                out["stream-digest" if digest else "stream"] = t.counted(pkg, s, c0)
                for k in range(3):
                    (q.pop_digest if digest else q.pop)()
                q.close()
        else:
            out[name] = t.render_batch(pkg, s, ch, nsamp, flags)[2]
print(json.dumps(out))
