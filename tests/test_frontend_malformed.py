"""The host front end (pluto-gps-sim_amd/host/gpsfe.c) on navigation and motion files that are damaged.  CPU only.

tools/fe_asan.c, a stand-alone C program, is built twice from gpsfe.c itself: with the host Makefile's product flags, and with
-fsanitize=address,undefined -fno-sanitize-recover=all.  Both run over the corpus of tests/rinex_mutants.py, one forked child
per case: gpsfe_open plain, with -T, and from 20 s before the roll-over to the second ephemeris set; on success three
gpsfe_next_block, gpsfe_generate of 310 more blocks (across a 30 s maintenance) on one thread and again on four, one echo and
ten blocks.  Every case must end by itself within the limit, with a
documented return code, no signal, no sanitizer report and no descriptor the GPU side's contract refuses; every named case must
also give the outcome written beside it in rinex_mutants.py.  Nothing here is loaded into Python under a sanitizer.

Time limit per case: 20 x the time the same build of the driver takes for the unmodified synth3540.14n, process start included,
and 2 s at the least; measured again on every run and printed.  As measured when this was written: 34 ms for the product build,
76 ms for the sanitized one, so 2 s for both.  The 1210 cases are spread over four driver processes per build (6 s and 11 s);
the whole file took 23 s, building the two drivers included."""
import os
import re
import subprocess
import time

import pytest

import rinex_mutants as rm
from conftest import GOLDEN, ROOT

HOST = os.path.join(ROOT, "pluto-gps-sim_amd", "host")
SHARDS = 4
BUILDS = ("product", "sanitized")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def product_flags():
    """CFLAGS of pluto-gps-sim_amd/host/Makefile, what libgpsfe.so is built with (less -fPIC; the include path made absolute)"""
    with open(os.path.join(HOST, "Makefile")) as f:
        line = next(l for l in f if l.startswith("CFLAGS"))
    flags = [w for w in line.split("=", 1)[1].split() if w != "-fPIC"]
    assert "-ffp-contract=off" in flags and "-fno-builtin" in flags and "-O2" in flags
    return [("-I" + os.path.join(ROOT, "include")) if w.startswith("-I") else w for w in flags]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """{build: (path of the driver, None) or (None, the reason there is none)}"""
    d = tmp_path_factory.mktemp("fe_drivers")
    cc = os.environ.get("CC", "gcc")
    src = [os.path.join(ROOT, "tools", "fe_asan.c"), os.path.join(HOST, "gpsfe.c")]
    out = {}
    for build in BUILDS:
        flags = product_flags()
        if build == "sanitized":
            flags = [w for w in flags if w != "-O2"] + SANITIZE
        exe = str(d / ("fe_" + build))
        r = subprocess.run([cc] + flags + src + ["-o", exe, "-lm", "-lz", "-lpthread"], capture_output=True, text=True)
        if r.returncode != 0 and build == "sanitized" and re.search(r"asan|ubsan|sanitize", r.stderr):
            out[build] = (None, "%s cannot link the sanitizer runtimes: %s" % (cc, r.stderr.strip().splitlines()[-1]))
            continue
        assert r.returncode == 0, r.stderr
        out[build] = (exe, None)
    return out


LINE = re.compile(r"^(\S+) (?:open=(-?\d+) sets=(\S+) valid=(\S+) openT=(-?\d+) openR=(-?\d+) )?end=(.*)$")


def run_driver(exe, dirs, limit_ms):
    """the driver over every directory at once; {file name: (open, sets, valid, openT, end, openR)} and what it wrote to stderr"""
    procs = [subprocess.Popen([exe, str(d), os.path.join(GOLDEN, "synth3540.14n"), str(limit_ms)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, errors="replace") for d in dirs]
    res, err = {}, ""
    for p in procs:
        so, se = p.communicate()
        assert p.returncode in (0, 1), se[-2000:]
        err += se
        for l in so.splitlines():
            m = LINE.match(l)
            assert m, l
            rcs = [None if m.group(k) is None else int(m.group(k)) for k in (2, 5, 6)]
            res[m.group(1)] = (rcs[0], m.group(3), m.group(4), rcs[1], m.group(7), rcs[2])
    return res, err


@pytest.fixture(scope="module")
def outcome(drivers, tmp_path_factory):
    """{build: (results, stderr, limit in ms, results of the three golden navigation files)} for every build there is"""
    base = tmp_path_factory.mktemp("fe_corpus")
    dirs = [base / ("shard%d" % k) for k in range(SHARDS)]
    for d in dirs:
        d.mkdir()
    for k, c in enumerate(rm.CASES):
        (dirs[k % SHARDS] / rm.file_name(c)).write_bytes(c.data)
    one = base / "one"
    one.mkdir()
    (one / "synth3540.n2").write_bytes(rm.V2)
    gold = base / "golden"
    gold.mkdir()
    for name, (ext, data) in rm.GOLDEN_NAV.items():
        (gold / (name.split(".")[0] + ext)).write_bytes(data)
    out = {}
    for build, (exe, _) in drivers.items():
        if exe is None:
            continue
        t0 = time.perf_counter()
        res, _ = run_driver(exe, [one], 60000)
        healthy_ms = (time.perf_counter() - t0) * 1e3
        assert res["synth3540.n2"][4] == "ok", res
        limit_ms = max(2000, int(20 * healthy_ms))
        t0 = time.perf_counter()
        res, err = run_driver(exe, dirs, limit_ms)
        print("%s build: unmodified file %.0f ms, limit %d ms, %d cases in %.1f s" % (build, healthy_ms, limit_ms, len(res), time.perf_counter() - t0))
        out[build] = (res, err, limit_ms, run_driver(exe, [gold], limit_ms)[0])
    return out


def stderr_of(err, fname):
    """what the driver's children wrote between "== fname" and the next case"""
    at = err.find("== %s\n" % fname)
    if at < 0:
        return ""
    end = err.find("\n== ", at + 1)
    return err[at:end if end > 0 else len(err)][:3000]


@pytest.mark.parametrize("build", BUILDS)
def test_every_case_ends_by_itself_with_a_documented_code_and_sound_descriptors(drivers, outcome, build):
    """The safety property, over the named and the seeded random cases."""
    if build not in outcome:
        pytest.skip(drivers[build][1])
    res, err, limit_ms, _ = outcome[build]
    bad = []
    for c in rm.CASES:
        f = rm.file_name(c)
        assert f in res, "the driver gave no line for %s" % f
        rc, _, _, rct, end, rcr = res[f]
        if end != "ok" or rc not in rm.DOCUMENTED or rct not in rm.DOCUMENTED or rcr not in rm.DOCUMENTED:
            bad.append("%s (%s): open=%s openT=%s openR=%s end=%s (limit %d ms)\n%s" % (c.name, f, rc, rct, rcr, end, limit_ms, stderr_of(err, f)))
    assert not bad, "%d of %d cases:\n%s" % (len(bad), len(rm.CASES), "\n".join(bad[:12]))
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err, err[-3000:]


@pytest.mark.parametrize("case", [c for c in rm.NAMED if c.expect is not None], ids=lambda c: c.name)
def test_named_case_has_its_stated_outcome(outcome, case):
    for build, (res, err, limit_ms, _) in outcome.items():
        f = rm.file_name(case)
        rc, sets, valid, rct, end, rcr = res[f]
        what = "%s, %s build: open=%s sets=%s valid=%s openT=%s openR=%s end=%s\n%s" % (case.name, build, rc, sets, valid, rct, rcr, end, stderr_of(err, f))
        assert end == "ok", what
        assert rc == rm.RC[case.expect] and rct == rm.RC[case.expect], what
        if case.expect != "OK":
            assert rcr == rm.RC[case.expect], what
        if case.sets is not None:
            assert (int(sets), tuple(int(v) for v in valid.split(","))) == (len(case.sets), case.sets), what


def test_golden_files_keep_their_sets(outcome):
    """Three sets of 32 valid satellites in each of the three golden navigation files: what the commit before the reader's
    checks gave (its gpsfe.c with gpsfe_eph_sets added, under this driver)."""
    for build, (_, _, _, gold) in outcome.items():
        assert sorted(gold) == ["dense3540.n2", "synth3540.n2", "synth3540_v3.n3"]
        for f, r in gold.items():
            assert r == (0, "3", "32,32,32", 0, "ok", 0), (build, f, r)


def test_header_terms_that_are_not_finite_read_as_a_header_without_them(pkg, tmp_path):
    """An ionosphere or UTC line with a value that is not finite leaves the ionosphere model at its default and page 18 unsent:
    the descriptors, navigation words included, are those of the same file with that line taken out."""
    pkg.build_frontend()
    site = (30.286502, 120.032669, 100.0)
    cases = [c for c in rm.NAMED if c.name[2:].startswith(" header ")]
    assert len(cases) == 24
    for c in cases:
        L = rm.L3 if c.ext == ".n3" else rm.L2
        i = next(k for k in range(L.header) if c.data.split(b"\n")[k] != L.lines[k])
        damaged, without = tmp_path / "damaged", tmp_path / "without"
        damaged.write_bytes(c.data)
        without.write_bytes(L.join(L.lines[:i] + L.lines[i + 1:]))
        got = []
        for path in (damaged, without, os.path.join(GOLDEN, "synth3540_v3.rnx" if c.ext == ".n3" else "synth3540.14n")):
            fe = pkg.FrontEnd(str(path), llh=site, max_chan=12, rinex3=c.ext == ".n3")
            got.append(fe.generate(5).tobytes())
            fe.close()
        assert got[0] == got[1], c.name
        assert got[0] != got[2], c.name  # (the sound file does use its ionosphere terms)


@pytest.mark.parametrize("name", ["v2 a header and nothing else", "v2 month 00", "v2 ecc 9.9D+01", "gzip cut at 18"])
def test_gpsbb_sim_refuses_a_navigation_file_without_a_usable_record(pkg, tmp_path, name):
    """gpsbb-sim -e: refused with a message and a non-zero exit before a GPU or the output file is touched"""
    pkg.build_frontend()
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    case = next(c for c in rm.NAMED if c.name == name)
    assert case.expect == "NAVFILE"
    nav = tmp_path / "damaged.14n"
    nav.write_bytes(case.data)
    out = tmp_path / "never.bin"
    r = subprocess.run([exe, "-e", str(nav), "-d", "1", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "navigation file" in r.stderr
    assert not out.exists()
