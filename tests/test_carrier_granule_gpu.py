"""The state granule is a property of the kind (ev_carr_log2, gpsbb_events.hip.h): behind the lap-parallel pre-pass the tile tables
hold one exact CODE state (and data-bit word) per 2^g tiles and one exact CARRIER state per 2^gc tiles, gc = min(g + 1, 2) for
g >= 1 — by default g = 1, gc = 2 — and k_synth_ev, the despreaders and the model-error replay derive every tile from the states of
its two granules.  Here, at the default and (a process of its own each) with GPSBB_EV_STATE_LOG2 = 0: the IQ and end states of
workloads whose blocks end inside a granule of either kind, whose chunks start at every place of a carrier granule, whose carriers
are fast, slow, mirrored onto 512 exactly, and whose code rolls over with a data-bit change where the two places differ, are
bit-identical to the CPU oracle — on the fast path and with nearly every lane-run sent down the exact path (GPSBB_EV_DANGER); the
exact path is not taken much more often than with one state per tile; the despreaders' sums do not depend on the granule; and the
tables the lap-parallel pre-pass leaves at the default digest like the row walks'."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = r"""
import ctypes, hashlib, json, os, sys
import numpy as np
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
from __graft_entry__ import load_package
import oracle_binding as ob
pkg = load_package()
orc = ob.Oracle()
L = pkg.lib()
L.gpsbb_test_state_log2.argtypes = [ctypes.c_void_p]
L.gpsbb_test_state_log2_carr.argtypes = [ctypes.c_void_p]

def base(nb, nch, fs, seed, fmax, sign=0.0):
    ch = pkg.synth_descriptors(nb, nch=nch, seed=seed, max_doppler=fmax)
    if sign:
        ch["f_carr"] = sign * np.abs(ch["f_carr"])
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    return ch, 1.0 / fs

def rollover(ch, delt, b, i, at, frac=0.5):
    # channel i of block b rolls over between samples at and at + 1, and the roll-over ends a data bit whose successor differs
    sc = ch["f_code"][b, i] * delt
    ch["code_phase"][b, i] = 1023.0 - sc * (at + frac)
    ch["icode"][b, i] = 19
    ch["ibit"][b, i] = 5
    ch["dwrd"][b, i, :] = 0x2AAAAAAA

def partial(nb, nch, nsamp, seed):
    ch, delt = base(nb, nch, 25e6, seed, 9000.0)
    return ch, delt

def fast(sign, seed):
    return base(4, 16, 25e6, seed, 12000.0, sign)

def mirrored():
    # falling carriers that start a block, and so a granule, at phase 0: mirrored, the granule state is 512 exactly
    ch, delt = base(3, 16, 25e6, 31, 9000.0, -1.0)
    ch["carr_phase"][:, :] = 0.0
    return ch, delt

def slow():
    ch, delt = base(3, 16, 25e6, 32, 5000.0)
    ch["f_carr"] = np.where(np.arange(16)[None, :] % 2 == 0, 0.5, -0.5)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    return ch, delt

def roll_r3():
    # tiles 3, 7 and 11: the carrier's place in its granule is 3, the code's 1
    ch, delt = base(2, 16, 25e6, 33, 9000.0)
    for b in range(2):
        for i, at in ((0, 3 * 1024 + 500), (1, 7 * 1024 + 3), (2, 11 * 1024 + 1020), (3, 7 * 1024 + 1023), (4, 3 * 1024)):
            rollover(ch, delt, b, i, at, 0.3 + 0.1 * i)
    return ch, delt

cases = [
    ("6 tiles and one sample, one block of 8", partial(1, 8, 5 * 1024 + 1, 21), 5 * 1024 + 1, 0),
    ("6 tiles and one sample, 5 chained blocks of 16", partial(5, 16, 5 * 1024 + 1, 22), 5 * 1024 + 1, pkg.CHAIN_CARRIER),
    ("4095 samples, one block of 8", partial(1, 8, 4095, 23), 4095, 0),
    ("4095 samples, 5 chained blocks of 16", partial(5, 16, 4095, 24), 4095, pkg.CHAIN_CARRIER),
    ("4 tiles and one sample, one block of 8", partial(1, 8, 4 * 1024 + 1, 25), 4 * 1024 + 1, 0),
    ("4 tiles and one sample, 5 chained blocks of 16", partial(5, 16, 4 * 1024 + 1, 26), 4 * 1024 + 1, pkg.CHAIN_CARRIER),
    ("rising carriers at the kc = 4 limit, chained", fast(1.0, 27), 99000, pkg.CHAIN_CARRIER),
    ("falling carriers at the kc = 4 limit, chained", fast(-1.0, 28), 99000, pkg.CHAIN_CARRIER),
    ("falling carriers mirrored onto 512 exactly", mirrored(), 20000, 0),
    ("carriers of 0.5 Hz, chained", slow(), 50001, pkg.CHAIN_CARRIER),
    ("roll-over and data-bit change at carrier place 3, code place 1", roll_r3(), 13 * 1024 + 7, pkg.CHAIN_CARRIER),
    ("16.368 MS/s, both signs, chained", base(3, 16, 16.368e6, 34, 7000.0), 80000, pkg.CHAIN_CARRIER),
]
DESPREAD = (1, 10)  # the cases whose despreader sums are compared
out = []
with pkg.Synth(0) as s:
    for k, (name, (ch, delt), nsamp, flags) in enumerate(cases):
        s.hazards(reset=True)
        b = s.batch(ch, delt, nsamp, flags=flags)
        b.run(); s.sync()
        iq, st = b.read()
        g, gc = int(L.gpsbb_test_state_log2(b._b)), int(L.gpsbb_test_state_log2_carr(b._b))
        w = {"name": name, "exact": int(s.info(pkg.INFO_EXACT_RUNS)), "kernel": int(s.info(pkg.INFO_LAST_KERNEL)),
             "prepass": int(s.info(pkg.INFO_PREPASS)), "g": g, "gc": gc}
        if k in DESPREAD:
            w["despread"] = hashlib.sha256(b.despread(seg_tiles=3).tobytes()).hexdigest()
            w["lags"] = hashlib.sha256(b.despread_lags([-2, 0, 3], seg_tiles=3).tobytes()).hexdigest()
        b.close()
        want_iq, want_st, _ = orc.fill_blocks(ch, delt, nsamp, chain=bool(flags & pkg.CHAIN_CARRIER))
        act = ch["prn"] > 0
        w["state_ok"] = all(st[f][act].tobytes() == want_st[f][act].tobytes()
                            for f in ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit"))
        w["iq_ok"] = bool((iq == want_iq).all())
        w["iq_sha"] = hashlib.sha256(iq.tobytes()).hexdigest()
        w["lane_runs"] = int(act.sum()) * ((nsamp + 15) // 16)
        out.append(w)
print(json.dumps(out))
"""


def run_child(**knobs):
    env = dict(os.environ, GPSBB_PY_LIB="exp")
    env.pop("GPSBB_EV_STATE_LOG2", None)  # (the default granules unless a knob says otherwise)
    env.update({k: str(v) for k, v in knobs.items()})
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def default_run():
    return run_child()


@pytest.fixture(scope="module")
def per_tile_run():
    return run_child(GPSBB_EV_STATE_LOG2=0)


def test_default_granules_are_two_tiles_of_code_and_four_of_carrier(default_run):
    for w in default_run:
        assert w["kernel"] == 2 and w["prepass"] == 3, w  # k_synth_ev behind the lap-parallel pre-pass
        assert (w["g"], w["gc"]) == (1, 2), w


def test_iq_and_end_states_are_the_oracles(default_run):
    for w in default_run:
        assert w["iq_ok"] and w["state_ok"], w


def test_exact_path_from_both_granules_renders_the_same_bits(default_run):
    """GPSBB_EV_DANGER raised: nearly every lane-run is recomputed by ev_exact_run, each NCO from the state of its own granule"""
    forced = run_child(GPSBB_EV_DANGER=0xF0000000)  # 15 / 16 of every tested quantity's low words are below it
    for w, w0 in zip(forced, default_run):
        assert (w["g"], w["gc"]) == (1, 2), w
        assert w["iq_ok"] and w["state_ok"] and w["iq_sha"] == w0["iq_sha"], w
        assert w["exact"] > w["lane_runs"] // 2, w  # (the knob took effect)


def test_exact_path_is_not_taken_much_more_often_than_with_a_state_per_tile(default_run, per_tile_run):
    for w, w0 in zip(default_run, per_tile_run):
        assert (w0["g"], w0["gc"]) == (0, 0), w0
        assert w0["iq_ok"] and w0["state_ok"] and w["iq_sha"] == w0["iq_sha"], w0
        assert w["exact"] <= 2 * w0["exact"] + 4, (w["name"], w["exact"], w0["exact"])


def test_despreaders_sums_do_not_depend_on_the_granule(default_run, per_tile_run):
    n = 0
    for w, w0 in zip(default_run, per_tile_run):
        if "despread" in w:
            assert w["despread"] == w0["despread"] and w["lags"] == w0["lags"], w["name"]
            n += 1
    assert n == 2


def test_default_tables_digest_like_the_row_walks():
    """tools/table_check.py at the default granules: the lap-parallel pre-pass's tables, the same with its references pushed off
    (GPSBB_LAP_JITTER), and the row walks' at the tiles that start a granule of their kind"""
    env = dict(os.environ)
    env.pop("GPSBB_EV_STATE_LOG2", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "table_check.py"), "--cases", "2", "--seed", "21"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "tables bit-identical in every mode" in r.stdout
