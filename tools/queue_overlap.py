#!/usr/bin/env python3
"""Which kernels ran on which hardware queue, and did the pre-pass run beside the synthesis?

Reads the kernel-trace CSV of one `rocprofv3 --kernel-trace` run of bench.py (queue id, start and end of every dispatch)
and prints one JSON object:

  queues             per hardware queue id: dispatches and busy milliseconds per kernel (template arguments kept, argument
                     lists dropped)
  synth_overlapped   the fraction of the synthesis kernel's run time during which at least one pre-pass kernel (k_lap_*) of
                     the same process was running
  synth_cover        pushes_per_step x avg(synthesis kernel) / ms_per_step: how much of a step the synthesis kernel covers
                     (only with --ms-per-step or --bench-json)

  python tools/queue_overlap.py TRACE.csv [--bench-json LINE.json | --ms-per-step MS] [--pushes-per-step 8]
                                [--synth k_synth_ev] [--prepass k_lap_]
"""
import argparse
import collections
import csv
import json
import re
import sys


def column(header, *names):
    low = {h.lower(): h for h in header}
    for n in names:
        if n.lower() in low:
            return low[n.lower()]
    raise SystemExit("no column of %s in %s" % (names, header))


def short_name(name):
    """`void k_lap_pass2<1, true, 1>(BatchDev, LapDev) [clone .kd]` -> `k_lap_pass2<1,true,1>`"""
    name = re.sub(r"\s*\[clone[^\]]*\]", "", name).strip()
    depth = 0
    for i, c in enumerate(name):  # cut at the argument list: the first '(' outside template brackets
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            name = name[:i]
            break
    name = name.split(" ")[-1] if "<" not in name else re.sub(r"^(void|int)\s+", "", name)
    name = name.replace(", ", ",").replace(".kd", "")
    head = name.split("<", 1)[0]
    return name[head.rfind("::") + 2:] if "::" in head else name  # without its namespace


def union(intervals):
    out = []
    for a, b in sorted(intervals):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def overlap_ns(synth, merged):
    """total length of (each synth interval) ∩ (union of pre-pass intervals); both sorted by start"""
    total, j = 0, 0
    for a, b in sorted(synth):
        while j > 0 and merged[j - 1][1] > a:
            j -= 1
        while j < len(merged) and merged[j][1] <= a:
            j += 1
        k = j
        while k < len(merged) and merged[k][0] < b:
            total += max(0, min(b, merged[k][1]) - max(a, merged[k][0]))
            k += 1
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace")
    ap.add_argument("--bench-json", help="file holding bench.py's result line (ms_per_step is read from it)")
    ap.add_argument("--ms-per-step", type=float)
    ap.add_argument("--pushes-per-step", type=int, default=8)
    ap.add_argument("--synth", default="k_synth_ev")
    ap.add_argument("--prepass", default="k_lap_")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()

    with open(args.trace, newline="") as f:
        rd = csv.DictReader(f)
        cq = column(rd.fieldnames, "Queue_Id", "queue_id")
        cn = column(rd.fieldnames, "Kernel_Name", "kernel_name", "Name")
        cs = column(rd.fieldnames, "Start_Timestamp", "start_timestamp", "BeginNs")
        ce = column(rd.fieldnames, "End_Timestamp", "end_timestamp", "EndNs")
        rows = [(r[cq], short_name(r[cn]), int(r[cs]), int(r[ce])) for r in rd]
    if not rows:
        raise SystemExit("no dispatches in %s" % args.trace)

    queues = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0]))
    for q, n, a, b in rows:
        queues[q][n][0] += 1
        queues[q][n][1] += b - a
    synth = [(a, b) for _, n, a, b in rows if n.startswith(args.synth)]
    pre = union([(a, b) for _, n, a, b in rows if n.startswith(args.prepass)])
    synth_ns = sum(b - a for a, b in synth)
    out = {
        "label": args.label or args.trace,
        "dispatches": len(rows),
        "queues": {q: {n: {"n": v[0], "ms": round(v[1] / 1e6, 3)} for n, v in sorted(ks.items(), key=lambda kv: -kv[1][1])}
                   for q, ks in sorted(queues.items())},
        "synth_kernel": args.synth, "synth_launches": len(synth),
        "synth_avg_ms": round(synth_ns / 1e6 / len(synth), 4) if synth else None,
        "synth_queues": sorted({q for q, n, _, _ in rows if n.startswith(args.synth)}),
        "prepass_queues": sorted({q for q, n, _, _ in rows if n.startswith(args.prepass)}),
        "synth_overlapped": round(overlap_ns(synth, pre) / synth_ns, 4) if synth_ns else None,
    }
    ms = args.ms_per_step
    if args.bench_json:
        for line in open(args.bench_json):
            line = line.strip()
            if line.startswith("{"):
                b = json.loads(line)
                ms = b.get("ms_per_step", ms)
                out["value"] = b.get("value")
                out["hw_queues"] = b.get("dist", {}).get("hw_queues")
                out["streams_of_the_handle"] = b.get("dist", {}).get("streams_of_the_handle")
    if ms and synth:
        out["ms_per_step"] = ms
        out["synth_cover"] = round(args.pushes_per_step * synth_ns / 1e6 / len(synth) / ms, 4)
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
