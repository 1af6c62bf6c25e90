#!/usr/bin/env python3
"""Per-launch averages of the rocprofv3 runs under one directory, as one JSON document: every sub-directory is one run (one
library, one counter — counters are collected in passes of their own, without tracing — or one --kernel-trace --stats run), named
<library>_<counter> or <library>_trace.

    python tools/pmc_kernels.py <directory> [kernel name fragment ...]

Counter values are what rocprofv3 reports (WRITE_SIZE / FETCH_SIZE: KiB), averaged over the dispatches of a kernel, as
tools/pmc_summary.py reads them; a trace run gives launches and the average duration in microseconds."""
import glob
import json
import os
import sqlite3
import sys


def short(name):
    """the kernel's own name with its template arguments: "k_synth_ev<1>" (rocprofv3: "[void ]gpsbb_impl::<name>(<args>)")"""
    return name.split("(")[0].split("::")[-1].strip().replace(", ", ",")


def rows(db, sql):
    c = sqlite3.connect(db)
    try:
        return list(c.execute(sql))
    finally:
        c.close()


def main():
    tag = sys.argv[1]
    want = sys.argv[2:] or ["k_synth_ev", "k_lap_pass2"]
    out = {}
    for d in sorted(glob.glob(os.path.join(tag, "*", ""))):
        run = os.path.basename(os.path.dirname(d))
        lib, _, what = run.partition("_")
        for db in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
            if what == "trace":
                for n, calls, avg in rows(db, "select name,total_calls,average from top_kernels"):
                    if any(w in n for w in want):
                        out.setdefault("kernel_us", {}).setdefault(short(n), {})[lib] = {"launches": calls, "avg_us": avg}
            else:
                sql = "select kernel_name, counter_name, count(*), avg(value) from counters_collection group by kernel_name, counter_name"
                for n, ctr, cnt, avg in rows(db, sql):
                    if any(w in n for w in want):
                        out.setdefault(ctr, {}).setdefault(short(n), {})[lib] = {"launches": cnt, "avg": avg}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
