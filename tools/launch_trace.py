#!/usr/bin/env python3
"""Do two builds of the library launch the same kernels, in the same order, on the same queues?

  run       the workload to trace: every host path that launches a pre-pass — one gpsbb_fill_block, a chained resident batch
            run three times, a four-push host-gather stream, one gpsbb_chain_carrier call (more blocks than one sub-batch
            holds), a chained batch of the per-sample kernel; then the last four again with OPT_SEED_WHERE 1 (the row walks).
            GPSBB_PY_LIB selects the build, as tools/ab_lib.sh does:
                rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_trace.py run
  list      TRACE.csv -> one line per dispatch, queue by queue (queues numbered by their first dispatch): kernel, grid, workgroup
  compare   A.csv B.csv -> "identical", or the first dispatches that differ on every queue (exit status 1)
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run():
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    from __graft_entry__ import load_package
    pkg = load_package()
    delt, nsamp, nch = 1.0 / 25e6, 20000, 5
    with pkg.Synth(0) as s:
        ch = pkg.synth_descriptors(1, nch=nch, seed=11)
        s.fill_block(ch[0], delt, nsamp)
        for where in (0, 1):
            s.set_option(pkg.OPT_SEED_WHERE, where)
            b = s.batch(pkg.synth_descriptors(6, nch=nch, seed=12), delt, nsamp, flags=pkg.CHAIN_CARRIER)
            for _ in range(3):
                b.run()
            s.sync()
            b.close()
            st = s.stream(nch, delt, nsamp, 3, depth=3, flags=pkg.CHAIN_CARRIER)
            chs = pkg.synth_descriptors(12, nch=nch, seed=13)
            for k in range(4):
                st.push(chs[3 * k:3 * k + 3], new_chain=(k == 0))
                if st.pending == 3:
                    st.pop()
            while st.pending:
                st.pop()
            st.close()
            s.chain_carrier(pkg.synth_descriptors(16384 + 40, nch=2, seed=14), delt, 4000)
            s.set_option(pkg.OPT_SYNTH_KERNEL, 1)
            b = s.batch(pkg.synth_descriptors(6, nch=nch, seed=15), delt, nsamp, flags=pkg.CHAIN_CARRIER)
            b.run()
            s.sync()
            b.close()
            s.set_option(pkg.OPT_SYNTH_KERNEL, 0)
        s.set_option(pkg.OPT_SEED_WHERE, 0)
    print("launch_trace: done (%s)" % pkg.LIB_PATH)


def dispatches(path):
    """{queue number: [(kernel, grid, workgroup), ...] in dispatch order}"""
    from queue_overlap import column, short_name
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        cq = column(rd.fieldnames, "Queue_Id", "queue_id")
        cn = column(rd.fieldnames, "Kernel_Name", "kernel_name", "Name")
        cd = column(rd.fieldnames, "Dispatch_Id", "dispatch_id", "Start_Timestamp")
        dims = [[column(rd.fieldnames, "%s_Size_%s" % (w, a), "%s_Size_%s" % (w.lower(), a.lower())) for a in "XYZ"]
                for w in ("Grid", "Workgroup")]
        rows = sorted(((int(r[cd]), r[cq], short_name(r[cn]), tuple(int(r[c]) for c in dims[0]), tuple(int(r[c]) for c in dims[1]))
                       for r in rd), key=lambda r: r[0])
    number, out = {}, {}
    for _, q, name, grid, wg in rows:
        out.setdefault(number.setdefault(q, len(number)), []).append((name, grid, wg))
    return out


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        return run()
    if len(sys.argv) == 3 and sys.argv[1] == "list":
        for q, ds in sorted(dispatches(sys.argv[2]).items()):
            for name, grid, wg in ds:
                print("q%d %s grid %s wg %s" % (q, name, "x".join(map(str, grid)), "x".join(map(str, wg))))
        return 0
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        a, b = dispatches(sys.argv[2]), dispatches(sys.argv[3])
        same = True
        for q in sorted(set(a) | set(b)):
            da, db = a.get(q, []), b.get(q, [])
            if da != db:
                same = False
                k = next((i for i, (x, y) in enumerate(zip(da, db)) if x != y), min(len(da), len(db)))
                print("q%d: %d / %d dispatches, first difference at %d: %s / %s" % (q, len(da), len(db), k, da[k:k + 1], db[k:k + 1]))
        if same:
            print("identical (%d dispatches on %d queues)" % (sum(len(v) for v in a.values()), len(a)))
        return 0 if same else 1
    raise SystemExit(__doc__)


if __name__ == "__main__":
    sys.exit(main())
