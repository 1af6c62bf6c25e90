"""Does a change leave bench.py's headline alone?  This tree's library against another build of it (the parent commit's) on one box
in one session: per round this tree's, the other's, this tree's again — the legs alternate and every round holds an A/A pair, two
runs apart, whose spread is the margin the A/B difference is read against.  Every leg is a fresh process; the first leg that
fails ends the session.

    python tools/ab_headline.py /path/to/parent/libgpsbb.so [--rounds 4] [--what "..."] [--json OUT]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu", "--no-extras"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--what", default="")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ab_headline.json"))
    a = ap.parse_args()
    other = os.path.abspath(a.other)
    out = {"what": a.what, "bench": "bench.py " + " ".join(BENCH), "bench_value_unit": "IQ samples/s",
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", ""), "order": [], "values": {}, "lines": {}}
    for r in range(1, a.rounds + 1):
        for leg in ("new a", "parent", "new b"):
            env = dict(os.environ)
            env.pop("GPSBB_PY_LIB", None)
            if leg == "parent":
                env["GPSBB_PY_LIB"] = other
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + BENCH, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=600)
            name = "%s %d" % (leg, r)
            if p.returncode != 0:
                sys.stderr.write(p.stderr.decode(errors="replace")[-4000:])
                sys.exit("%s: bench.py exit status %d" % (name, p.returncode))
            line = json.loads(p.stdout.decode().strip().splitlines()[-1])
            out["order"].append(name)
            out["values"][name] = line["value"]
            out["lines"][name] = {k: line[k] for k in ("value", "ms_per_step", "steps", "warmup") if k in line}
            if "roofline" in line:
                out["lines"][name]["kernel_ms_per_launch"] = line["roofline"].get("ms_per_launch")
            print("%-9s %.6g" % (name, line["value"]), flush=True)
    v = out["values"]
    new = [v[k] for k in out["order"] if k.startswith("new")]
    par = [v[k] for k in out["order"] if k.startswith("parent")]
    aa = [abs(v["new a %d" % r] - v["new b %d" % r]) / v["new a %d" % r] for r in range(1, a.rounds + 1)]
    out["summary"] = {"new_median": statistics.median(new), "parent_median": statistics.median(par), "new_min": min(new), "new_max": max(new),
                      "parent_min": min(par), "parent_max": max(par), "new_over_parent": statistics.median(new) / statistics.median(par),
                      "aa_spread_max": max(aa), "aa_spread_median": statistics.median(aa)}
    print(json.dumps(out["summary"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
