#!/usr/bin/env python3
"""Record the byte layout of the reference's channel_t in tests/golden/ref_channel_t_layout.json.

    python tests/golden/make_ref_layout.py REFERENCE_DIR

A C program including REFERENCE_DIR/plutogpssim.h prints offsetof() of every field gpsbb_fill_block_ref touches, plus
sizeof(channel_t), the size of a dwrd element and of carr_phase; once as the header stands (FLOAT_CARR_PHASE) and once with
line 12 (`#define FLOAT_CARR_PHASE`) taken out in a temporary copy - the reference's other channel_t (h:160-161), the layout
gpsbb_fill_block_ref_fixed reads.  The JSON it writes is committed: tests/test_ref_layout.py checks the package's
REF_CHANNEL_DTYPE / REF_CHANNEL_FIXED_DTYPE against it without the header."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_channel_t_layout.json")
FIELDS = ["prn", "ca", "f_carr", "f_code", "carr_phase", "code_phase", "g0", "sbf", "dwrd", "iword", "ibit", "icode",
          "dataBit", "codeCA", "azel", "rho0"]


def layout(hdr, fixed, tmp):
    fields = list(FIELDS)
    if fixed:
        lines = open(hdr).read().splitlines(True)
        assert lines[11].startswith("#define FLOAT_CARR_PHASE")
        hdr = os.path.join(tmp, "plutogpssim_fixed.h")
        open(hdr, "w").write("".join(lines[:11] + lines[12:]))
        fields.insert(fields.index("carr_phase") + 1, "carr_phasestep")
    src = os.path.join(tmp, "off.c")
    body = "\n".join('    printf("%s %%zu\\n", offsetof(channel_t, %s));' % (f, f) for f in fields)
    open(src, "w").write('#include <stdbool.h>\n#include <limits.h>\n#include <stddef.h>\n#include <stdint.h>\n#include <stdio.h>\n'
                         '#include <sys/types.h>\n#include "%s"\nint main(void) {\n%s\n'
                         '    printf("sizeof %%zu\\n", sizeof(channel_t));\n'
                         '    printf("sizeof_dwrd_elem %%zu\\n", sizeof(((channel_t *)0)->dwrd[0]));\n'
                         '    printf("sizeof_carr_phase %%zu\\n", sizeof(((channel_t *)0)->carr_phase));\n    return 0;\n}\n' % (hdr, body))
    exe = os.path.join(tmp, "off")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", src, "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    return {"offsets": {f: int(got[f]) for f in fields}, "sizeof": int(got["sizeof"]),
            "sizeof_dwrd_elem": int(got["sizeof_dwrd_elem"]), "sizeof_carr_phase": int(got["sizeof_carr_phase"])}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    hdr = os.path.join(sys.argv[1], "plutogpssim.h")
    with tempfile.TemporaryDirectory() as tmp:
        res = {"float_carr_phase": layout(hdr, False, tmp), "fixed_carr_phase": layout(hdr, True, tmp)}
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
