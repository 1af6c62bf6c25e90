#!/usr/bin/env python3
"""Is the device code of two builds the same?  Compares two outputs of `make -C pluto-gps-sim_amd/csrc asm` (the device
assembly -save-temps leaves, gpsbb-hip-amdgcn-amd-amdhsa-gfx950.s), kernel by kernel, whatever order the functions come in:
the set of kernel symbols, every kernel's instructions from its label to the end of the function (block labels renumbered,
comments dropped) and its .amdhsa_kernel descriptor (registers, LDS, scratch).

    python tools/asm_same.py PARENT.s THIS.s [PARENT.log THIS.log]  ->  "identical: N kernels ...", or what differs (exit status 1)

With the two logs of those builds as well: the -Rpass-analysis=kernel-resource-usage remarks, function by function.
"""
import re
import sys


def kernels(path):
    """{symbol: (instructions, descriptor lines)}, and the symbols in file order"""
    lines = open(path, errors="replace").read().split("\n")
    desc, body, order = {}, {}, []
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i + 1
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[m.group(1)] = [" ".join(l.split()) for l in lines[i + 1:j]]
            i = j
        i += 1
    for sym in desc:
        start = next(k for k, l in enumerate(lines) if l.startswith(sym + ":"))
        order.append((start, sym))
        out = []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";", 1)[0].rstrip()
            if l:
                out.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(l.split())))
        body[sym] = out
    return body, desc, [s for _, s in sorted(order)]


def remarks(path):
    """{function: its kernel-resource-usage remarks, without file positions}"""
    out, cur = {}, None
    for l in open(path, errors="replace"):
        m = re.match(r"remark: [^ ]*: +(.*?) \[-Rpass-analysis=kernel-resource-usage\]", l)
        if not m:
            continue
        if m.group(1).startswith("Function Name:"):
            cur = out.setdefault(m.group(1).split(":", 1)[1].strip(), [])
        elif cur is not None:
            cur.append(m.group(1))
    return out


def main():
    if len(sys.argv) not in (3, 5):
        raise SystemExit(__doc__)
    (ba, da, oa), (bb, db, ob) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for s in sorted(set(ba) ^ set(bb)):
        print("only in %s: %s" % (sys.argv[1] if s in ba else sys.argv[2], s))
        bad += 1
    for s in sorted(set(ba) & set(bb)):
        if ba[s] != bb[s]:
            print("instructions differ: %s (%d / %d lines)" % (s, len(ba[s]), len(bb[s])))
            bad += 1
        if da[s] != db[s]:
            print("descriptor differs: %s: %s" % (s, sorted(set(da[s]) ^ set(db[s]))))
            bad += 1
    if len(sys.argv) == 5:
        ra, rb = remarks(sys.argv[3]), remarks(sys.argv[4])
        for s in sorted(set(ra) | set(rb)):
            if ra.get(s) != rb.get(s):
                print("resource usage differs: %s: %s / %s" % (s, ra.get(s), rb.get(s)))
                bad += 1
        if not bad:
            print("resource usage: %d functions, every figure equal" % len(ra))
    if bad:
        return 1
    print("identical: %d kernels, %d instruction lines, every .amdhsa_kernel descriptor; functions in %s order"
          % (len(ba), sum(len(v) for v in ba.values()), "the same" if oa == ob else "a different"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
