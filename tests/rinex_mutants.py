"""Damaged navigation and motion files for the host front end, each with the outcome it must have: the corpus of
tests/test_frontend_malformed.py, which runs tools/fe_asan.c over it.  Built once at import, deterministically, from the
committed files of tests/golden/; nothing of it is committed.  A plain helper, not a conftest.

A case is (name, ext, data, expect, sets):
  ext     ".n2" a navigation file for the RINEX 2 reader, ".n3" for the RINEX 3 reader, ".csv" a motion file
  expect  "OK", "NAVFILE" or "MOTION": what gpsfe_open must return, plain and with -T; None for the seeded random cases,
          which are held to the safety property only (ends by itself, a documented return code, no signal, no sanitizer
          report, no descriptor that is not fit to render)
  sets    the valid satellites of every ephemeris set, where expect is "OK" and the file is a navigation file

The expectations are written down from the policy of include/gpsfe.h (GPSFE_E_NAVFILE, GPSFE_E_MOTION), not from what the
front end gives:
  * a record is taken only if it is complete (eight lines), finite and within the navigation message's ranges; reading stops
    at the first that is not, the sets read so far are used, no valid record at all is GPSFE_E_NAVFILE;
  * a field that is blank or cut off reads 0, as in the reference.  So a line of a record that is emptied or cut passes unless
    it is the record's first line cut before its date is complete (month 0), or the line that holds sqrt(A) (0 is refused);
    the eighth line holds nothing the front end uses, so a file cut inside it loses nothing;
  * the RINEX 3 reader skips every line that does not begin with G (other constellations): there an emptied first line takes
    its record out and reading goes on;
  * the golden files hold three sets (00:00, 02:00, 04:00) of 32 satellites, in the order of the PRNs."""
import gzip
import os
import random
import zlib
from collections import namedtuple

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Case = namedtuple("Case", "name ext data expect sets")

RC = {"OK": 0, "NAVFILE": -2, "MOTION": -3}
DOCUMENTED = (0, -1, -2, -3, -4, -5, -6)  # GPSFE_OK and the GPSFE_E_* of include/gpsfe.h

FULL = (32, 32, 32)
LAST_LOST = (32, 32, 31)
FIRST_LOST = (31, 32, 32)


def _read(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


V2 = _read("synth3540.14n")
V2_DENSE = _read("dense3540.14n")
V3 = _read("synth3540_v3.rnx")
MOTION = _read("circle_motion.csv")
GOLDEN_NAV = {"synth3540.14n": (".n2", V2), "dense3540.14n": (".n2", V2_DENSE), "synth3540_v3.rnx": (".n3", V3)}


class Layout:
    """Where things are in a golden file: `o` the column shift of the 19-character fields, the columns of PRN and month."""

    def __init__(self, tag, ext, data, o, prn_col, month_col, is_record):
        self.tag, self.ext, self.data, self.o, self.prn_col, self.month_col = tag, ext, data, o, prn_col, month_col
        self.lines = data.split(b"\n")[:-1]  # the file ends with a line feed
        self.header = next(i for i, l in enumerate(self.lines) if l[60:73] == b"END OF HEADER") + 1
        self.records = [i for i in range(self.header, len(self.lines)) if is_record(self.lines[i])]
        self.first, self.last = self.records[0], self.records[-1]

    def join(self, lines):
        return b"\n".join(lines) + b"\n"

    def with_line(self, i, new):
        lines = list(self.lines)
        lines[i] = new
        return self.join(lines)

    def with_cols(self, i, col, text):
        l = self.lines[i]
        return self.with_line(i, l[:col] + text + l[col + len(text):])

    def with_field(self, i, k, text):
        """field k (0..3) of line i: 19 characters from column 3 + o + 19 k"""
        return self.with_cols(i, 3 + self.o + 19 * k, text.rjust(19).encode())

    def offset(self, i):
        """byte offset of line i"""
        return sum(len(l) + 1 for l in self.lines[:i])


L2 = Layout("v2", ".n2", V2, 0, 0, 6, lambda l: l[:2].strip().isdigit() and l[2:3] == b" " and l[3:5] == b"14")
L3 = Layout("v3", ".n3", V3, 1, 1, 9, lambda l: l[:1] == b"G")
assert len(L2.records) == 96 and len(L3.records) == 96 and L2.header == 8 and L3.header == 8

ORBIT2 = 2  # the record's line with eccentricity (field 1) and sqrt(A) (field 3)


def named_cases():
    c = []

    def add(name, ext, data, expect, sets=None):
        c.append(Case(name, ext, data, expect, sets if expect == "OK" and ext != ".csv" else None))

    for L in (L2, L3):
        t = L.tag
        # month columns, in the first record (nothing is left) and in the last (everything before it is)
        for mm in (b"00", b"13", b"75"):
            add("%s month %s" % (t, mm.decode()), L.ext, L.with_cols(L.first, L.month_col, mm), "NAVFILE")
            add("%s month %s in the last record" % (t, mm.decode()), L.ext, L.with_cols(L.last, L.month_col, mm), "OK", LAST_LOST)
        # a trailing blank line: month 0 under the RINEX 2 reader, a line without G under the RINEX 3 reader
        add("%s trailing blank line" % t, L.ext, L.data + b"\n", "OK", FULL)
        add("%s trailing line of blanks" % t, L.ext, L.data + b" " * 80 + b"\n", "OK", FULL)
        # the file cut inside each line of the first and of the last record (40 characters in)
        for k in range(8):
            add("%s cut inside line %d of the first record" % (t, k + 1), L.ext, L.data[:L.offset(L.first + k) + 40],
                "OK" if k == 7 else "NAVFILE", (1,))
            add("%s cut inside line %d of the last record" % (t, k + 1), L.ext, L.data[:L.offset(L.last + k) + 40],
                "OK", FULL if k == 7 else LAST_LOST)
        # eccentricity and sqrt(A)
        for v in ("1.0D+00", "9.9D+01", "-1.0D-02", "NaN", "Inf", "1.0D+999", "5.0D-01"):
            add("%s ecc %s" % (t, v), L.ext, L.with_field(L.first + ORBIT2, 1, v), "NAVFILE")
        add("%s ecc 4.9D-01" % t, L.ext, L.with_field(L.first + ORBIT2, 1, "4.9D-01"), "OK", FULL)
        for v in ("0.0", "-5.153D+03", "8.192D+03", "NaN"):
            add("%s sqrta %s" % (t, v), L.ext, L.with_field(L.first + ORBIT2, 3, v), "NAVFILE")
        # time of ephemeris: -T adds the shift to it and reduces the sum week by week, which never ends for Inf
        for v in ("Inf", "1.0D+300", "-1.6D+01", "6.048D+05"):
            add("%s toe %s" % (t, v), L.ext, L.with_field(L.first + 3, 0, v), "NAVFILE")
        # a value that is not finite in one field of every line (fields 1..3 of the first line: the clock terms)
        for k in range(8):
            for v in ("NaN", "-Inf"):
                add("%s %s in line %d" % (t, v, k + 1), L.ext, L.with_field(L.first + k, 1 + (k + 1) % 3, v), "NAVFILE")
                add("%s %s in line %d of the last record" % (t, v, k + 1), L.ext, L.with_field(L.last + k, 1 + k % 3, v), "OK", LAST_LOST)
        # PRN
        for p in (b"00", b"33", b"99"):
            add("%s prn %s" % (t, p.decode()), L.ext, L.with_cols(L.first, L.prn_col, p), "NAVFILE")
        # a line longer than the reader's buffer: its tail must not be read as the record's next line
        long_line = L.lines[L.first + 1] + b" " * 150 + L.lines[L.first + ORBIT2][:80] * 2
        assert len(long_line) > 300
        add("%s line of %d characters" % (t, len(long_line)), L.ext, L.with_line(L.first + 1, long_line), "NAVFILE")
        add("%s line of %d characters in the last record" % (t, len(long_line)), L.ext, L.with_line(L.last + 1, long_line), "OK", LAST_LOST)
        # whole-file damage
        nul = L.with_cols(L.first + ORBIT2, 22, b"\0\0\0")  # the line reads as cut there: no sqrt(A)
        add("%s NUL bytes inside a line" % t, L.ext, nul, "NAVFILE")
        add("%s CRLF line ends" % t, L.ext, L.data.replace(b"\n", b"\r\n"), "OK", FULL)
        add("%s no END OF HEADER" % t, L.ext, L.join(L.lines[:L.header - 1] + L.lines[L.header:]), "NAVFILE")
        add("%s a header and nothing else" % t, L.ext, L.join(L.lines[:L.header]), "NAVFILE")
        add("%s an empty file" % t, L.ext, b"", "NAVFILE")
        add("%s 500 NUL bytes" % t, L.ext, b"\0" * 500, "NAVFILE")
        add("%s file through the other reader" % t, ".n3" if L.ext == ".n2" else ".n2", L.data, "NAVFILE")

    # each line of the first record emptied and cut, RINEX 2 columns: fields end at 22, 41 and 60
    for k in range(8):
        for n in (0, 1, 3, 22, 41, 60):
            refused = (k == 0 and n < 22) or k == ORBIT2
            add("v2 line %d of the first record cut to %d" % (k + 1, n), ".n2", L2.with_line(L2.first + k, L2.lines[L2.first + k][:n]),
                "NAVFILE" if refused else "OK", FULL)
    # the same under the RINEX 3 reader, whose fields end one column later: a cut takes the last digit of an exponent, and what
    # that does to a value is not written down here.  Safety only, but for the two that are plain:
    for k in range(8):
        for n in (0, 1, 3, 22, 41, 60):
            data = L3.with_line(L3.first + k, L3.lines[L3.first + k][:n])
            if k == 0 and n == 0:
                add("v3 line 1 of the first record cut to 0", ".n3", data, "OK", FIRST_LOST)  # no G: skipped with its seven lines
            elif k == 0 and n in (1, 3):
                add("v3 line 1 of the first record cut to %d" % n, ".n3", data, "NAVFILE")    # PRN 0 / year 0
            else:
                c.append(Case("v3 line %d of the first record cut to %d" % (k + 1, n), ".n3", data, None, None))

    # more sets than the table holds: the file's three sets five times, six hours on each time
    lines = list(L2.lines[:L2.header])
    for rep in range(5):
        for i in L2.records:
            hour = int(L2.lines[i][12:14]) + 6 * rep
            epoch = L2.lines[i][:9] + b"%2d %2d" % (20 + hour // 24, hour % 24) + L2.lines[i][14:]
            lines += [epoch] + L2.lines[i + 1:i + 8]
    add("v2 fifteen sets", ".n2", L2.join(lines), "OK", (32,) * 13)

    # header: ionosphere and UTC terms that are not finite leave the model at its default; the records are read as ever
    def header_line(L, label, start):
        return next(i for i in range(L.header) if L.lines[i][60:].startswith(label) and L.lines[i].startswith(start))

    for L, label, start, col, width in ((L2, b"ION ALPHA", b"", 2, 12), (L2, b"ION BETA", b"", 14, 12), (L2, b"DELTA-UTC", b"", 3, 19),
                                        (L2, b"DELTA-UTC", b"", 22, 19), (L3, b"IONOSPHERIC CORR", b"GPSA", 5, 12),
                                        (L3, b"IONOSPHERIC CORR", b"GPSB", 17, 12), (L3, b"TIME SYSTEM CORR", b"GPUT", 5, 17),
                                        (L3, b"TIME SYSTEM CORR", b"GPUT", 22, 16)):
        i = header_line(L, label, start)
        for v in ("NaN", "Inf", "1.0D+999"):
            add("%s header %s column %d %s" % (L.tag, (start or label).decode(), col, v), L.ext,
                L.with_cols(i, col, v.rjust(width).encode()), "OK", FULL)

    # gzip of the RINEX 2 file, cut: the reader gets the text that inflates from what is there
    gz = gzip.compress(V2, mtime=0)
    for what, n in (("0", 0), ("10", 10), ("18", 18), ("the middle", len(gz) // 2), ("one byte short", len(gz) - 1)):
        text = zlib.decompressobj(31).decompress(gz[:n]) if n else b""
        assert V2.startswith(text)
        # records whose eighth line has begun are complete (see the module text), in the file's order: 32 per set
        got = text.split(b"\n")[L2.header:]
        nrec = sum(1 for r in range(96) if 8 * r + 7 < len(got) and got[8 * r + 7] != b"")
        sets = tuple(min(32, nrec - 32 * s) for s in range(3) if nrec > 32 * s)
        add("gzip cut at %s" % what, ".n2", gz[:n], "OK" if nrec else "NAVFILE", sets)
    add("gzip whole", ".n2", gz, "OK", FULL)

    # motion files
    m = MOTION.split(b"\n")
    add("motion empty", ".csv", b"", "MOTION")
    add("motion a single line", ".csv", m[0] + b"\n", "OK")
    add("motion a single line without a line feed", ".csv", m[0], "OK")
    add("motion no line feeds", ".csv", MOTION.replace(b"\n", b" "), "MOTION")
    add("motion a line of 5000 characters", ".csv", m[0] + b" " * 5000 + b"\n" + b"\n".join(m[1:]), "MOTION")
    add("motion a line of 5000 characters later", ".csv", b"\n".join(m[:5]) + b"\n" + b"7" * 5000 + b"\n" + b"\n".join(m[5:]), "OK")
    for what, line in (("nan", b"0.0,nan,1.0,2.0"), ("inf", b"0.0,1.0,-inf,2.0"), ("1e999", b"0.0,1.0,2.0,1e999"), ("nan time", b"nan,1.0,2.0,3.0"),
                       ("an empty field", b"0.0,,1.0,2.0"), ("three fields", b"0.0,1.0,2.0"), ("1.7e308", b"0.0,0.0,0.0,1.7e308")):
        add("motion %s in the first line" % what, ".csv", line + b"\n" + MOTION, "MOTION")
        add("motion %s in the sixth line" % what, ".csv", b"\n".join(m[:5]) + b"\n" + line + b"\n" + b"\n".join(m[5:]), "OK")
    return c


ALPHABET = b"0123456789 -+.DEe\nG\x00\xff"


def random_cases():
    """Per golden navigation file: 200 byte-flip mutants (50 seeds each of 1, 3, 20 and 200 positions) and a truncation every
    67 bytes through the first 6000 and the last 700 bytes (101 of them)."""
    c = []
    for fname in sorted(GOLDEN_NAV):
        ext, data = GOLDEN_NAV[fname]
        tag = fname.split(".")[0] + ("_v2" if ext == ".n2" else "")
        for nflip in (1, 3, 20, 200):
            for seed in range(50):
                rng = random.Random(1000 * nflip + seed)
                b = bytearray(data)
                for _ in range(nflip):
                    b[rng.randrange(len(b))] = ALPHABET[rng.randrange(len(ALPHABET))]
                c.append(Case("%s flip %d seed %d" % (tag, nflip, seed), ext, bytes(b), None, None))
        for n in list(range(0, 6000, 67)) + list(range(len(data) - 700, len(data), 67)):
            c.append(Case("%s truncated at %d" % (tag, n), ext, data[:n], None, None))
    return c


def file_name(case):
    return "".join(ch if ch.isalnum() or ch in "+-." else "_" for ch in case.name) + case.ext


NAMED = named_cases()
RANDOM = random_cases()
CASES = NAMED + RANDOM
assert len({file_name(c) for c in CASES}) == len(CASES)
