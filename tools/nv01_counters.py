#!/usr/bin/env python3
"""The exact-run and hazard counters of the cases of tests/test_nav_sign_gpu.py on the library GPSBB_PY_LIB names (the parent
commit's libgpsbb.so: what the test's PARENT table records), as one JSON line: "case run" -> [exact runs, itable_512, dwrd_oob,
tiles rendered, the library's IQ and end states are the oracle's].
    GPSBB_PY_LIB=/path/to/parent/libgpsbb.so python tools/nv01_counters.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import oracle_binding  # noqa: E402
import test_ev_tile_prologue_gpu as tp  # noqa: E402
import test_nav_sign_gpu as t  # noqa: E402

pkg = conftest.load_package()
oracle = oracle_binding.Oracle()
out = {"lib": pkg.LIB_PATH}
with pkg.Synth(0) as s:
    for case in t.CASES:
        ch, nsamp, want_iq, want_st, hz = t.wanted(pkg, oracle, case)
        for run in t.RUNS:
            iq, st, got, dig = t.render(pkg, s, ch, nsamp, run)
            out["%s %s" % (case, run)] = list(got) + [bool((iq == want_iq).all() and tp.same_states(st, want_st, ch) == [])]
    s.set_option(pkg.OPT_SYNTH_KERNEL, 0)
print(json.dumps(out))
