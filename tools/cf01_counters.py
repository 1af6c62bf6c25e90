#!/usr/bin/env python3
"""The exact-run and hazard counters of the cases of tests/test_ev_chip_flags_gpu.py on the library GPSBB_PY_LIB names (the
parent commit's libgpsbb.so: what the test's PARENT table records), as one JSON line: "case instance" -> [exact runs,
itable_512, dwrd_oob, tiles rendered], and whether the library's IQ is the oracle's.
    GPSBB_PY_LIB=/path/to/parent/libgpsbb.so python tools/cf01_counters.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import oracle_binding  # noqa: E402
import test_ev_chip_flags_gpu as t  # noqa: E402

pkg = conftest.load_package()
oracle = oracle_binding.Oracle()
out = {"lib": pkg.LIB_PATH}
with pkg.Synth(0) as s:
    for name in t.PARENT:
        case, inst = name.split()
        iq, st, got, variant, dig = t.render(pkg, s, case, inst)
        want_iq = t.wanted(pkg, oracle, case, inst)[0]
        out[name] = list(got) + [int(variant), bool((iq == want_iq).all())]
print(json.dumps(out))
