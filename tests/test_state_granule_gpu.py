"""The state granule of k_synth_ev (BatchDev::st_log2): behind the lap-parallel pre-pass the tile tables hold one exact state per
2^g tiles and the synthesis kernel derives the anchors of the tiles in between (gpsbb_events.hip.h).  Here, for g = 0, 1, 2 (the
experiments build, GPSBB_EV_STATE_LOG2 in a process of its own each): the IQ and end states of corner workloads are bit-identical
to the CPU oracle, the exact path is not taken much more often than with one state per tile, and every granule state the
lap-parallel pre-pass writes is the row walks' state of the same tile."""
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

def corner(nb, nch, fs, nsamp, seed, fmax, sign=0.0):
    ch = pkg.synth_descriptors(nb, nch=nch, seed=seed, max_doppler=fmax)
    rng = np.random.default_rng(seed)
    if sign:
        ch["f_carr"] = sign * np.abs(ch["f_carr"])
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    delt = 1.0 / fs
    # code roll-overs placed in the first tile of a 4-tile granule and in its last (samples 4096 k + 5, 4096 k + 3 * 1024 + 1000)
    for b in range(nb):
        for i, at in ((0, 4096 + 5), (1, 4096 * 2 + 3 * 1024 + 1000), (2, 4096 + 1024 + 7)):
            if i < nch:
                sc = ch["f_code"][b, i] * delt
                ch["code_phase"][b, i] = 1023.0 - sc * (at + rng.uniform(0.1, 0.9))
    return ch, delt

cases = [
    ("rising carriers at the kc = 4 limit, chained", corner(4, 16, 25e6, 99000, 11, 12000.0, 1.0), 99000, pkg.CHAIN_CARRIER),
    ("falling carriers at the kc = 4 limit, chained", corner(4, 16, 25e6, 99000, 12, 12000.0, -1.0), 99000, pkg.CHAIN_CARRIER),
    ("both signs, independent blocks, partial last granule", corner(5, 12, 25e6, 50001, 13, 9000.0), 50001, 0),
    ("16.368 MS/s, both signs, chained", corner(3, 16, 16.368e6, 80000, 14, 7000.0), 80000, pkg.CHAIN_CARRIER),
    ("one block of 4095 samples", corner(1, 8, 25e6, 4095, 15, 5000.0), 4095, 0),
]
out = []
with pkg.Synth(0) as s:
    for name, (ch, delt), nsamp, flags in cases:
        s.hazards(reset=True)
        b = s.batch(ch, delt, nsamp, flags=flags)
        b.run(); s.sync()
        iq, st = b.read()
        g = int(L.gpsbb_test_state_log2(b._b))
        b.close()
        want_iq, want_st, _ = orc.fill_blocks(ch, delt, nsamp, chain=bool(flags & pkg.CHAIN_CARRIER))
        act = ch["prn"] > 0
        same_st = all(st[f][act].tobytes() == want_st[f][act].tobytes() for f in ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit"))
        out.append({"name": name, "iq_ok": bool((iq == want_iq).all()), "state_ok": bool(same_st),
                    "iq_sha": hashlib.sha256(iq.tobytes()).hexdigest(), "exact": int(s.info(pkg.INFO_EXACT_RUNS)),
                    "kernel": int(s.info(pkg.INFO_LAST_KERNEL)), "prepass": int(s.info(pkg.INFO_PREPASS)), "st_log2": g})
print(json.dumps(out))
"""


def run_child(g):
    env = dict(os.environ, GPSBB_PY_LIB="exp", GPSBB_EV_STATE_LOG2=str(g))
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_granules_of_1_2_and_4_tiles_render_the_same_bits():
    runs = {g: run_child(g) for g in (0, 1, 2)}
    for g, res in runs.items():
        for w in res:
            assert w["kernel"] == 2 and w["prepass"] == 3 and w["st_log2"] == g, (g, w)  # the granule asked for is the one in force
            assert w["iq_ok"] and w["state_ok"], (g, w)
    for k, w0 in enumerate(runs[0]):
        for g in (1, 2):
            w = runs[g][k]
            assert w["iq_sha"] == w0["iq_sha"], (g, w["name"])
            # the same W and danger threshold: a longer model stretch may graze an integer a little more often, no more
            assert w["exact"] <= 2 * w0["exact"] + 4, (g, w["name"], w["exact"], w0["exact"])


@pytest.mark.parametrize("g", [0, 1, 2])
def test_granule_states_are_the_row_walks_states_of_their_tiles(g):
    """tools/table_check.py with the granule forced: the lap-parallel pre-pass's tables (one state per 2^g tiles) against the
    row walks' (one per tile) at the tiles that start a granule, and against the same pre-pass with its references pushed off;
    g = 0: every tile of every batch."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "table_check.py"), "--cases", "3", "--seed", "9"],
                       env=dict(os.environ, GPSBB_EV_STATE_LOG2=str(g)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "tables bit-identical in every mode" in r.stdout
