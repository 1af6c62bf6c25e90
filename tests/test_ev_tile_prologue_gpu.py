"""The tile prologue of k_synth_ev (synth_ev_body, pluto-gps-sim_amd/csrc/gpsbb_events.hip.h): a tile's anchor and data bits are
derived from its granule's exact state in the epilogue of the tile before it — the chain steps out of LDS, tile 0 of a granule
without the step, the roll-over fix-up only for the tiles behind it — and every tile still on its own, whichever tiles a wavefront
is handed and in what order.  16 channels at 25 MS/s, bit for bit against the CPU oracle (IQ and end states); where a case has
more blocks than the oracle has time for, every block's device digest against the per-sample kernel (OPT_SYNTH_KERNEL 1).

Every case also asserts: the batch's state granule is 1 (two tiles per exact state; asked of the experiments build, which has the
hook, for the same descriptors), the kernel that rendered is the breakpoint kernel proper, GPSBB_INFO_TILES_RENDERED grew by
blocks x tiles exactly, the hazard counters are the oracle's, and the hazard and exact-run counters are those the kernel gave for
the same input BEFORE the prologue was reworked (PARENT below; the anchors are bit-identical, so the lanes that take the exact
path are the same lanes).

PARENT was measured on an MI355X with the parent commit's library
(`GPSBB_PY_LIB=<the parent's libgpsbb.so> python tools/tp01_counters.py`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FS = 25e6
DELT = 1.0 / FS
TILE = 1024
STATE_FIELDS = ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA")

# exact-run and hazard counters of the parent commit's kernel for the cases below (name -> exact runs, itable_512, dwrd_oob)
PARENT = {
    "tiles-1024": (0, 0, 0),
    "tiles-3112": (0, 0, 0),
    "tiles-4096": (0, 0, 0),
    "tiles-9232": (0, 0, 0),
    "rollover": (0, 0, 0),
    "carriers-16": (2, 0, 0),
    "carriers-3": (0, 0, 0),
    "chunks-of-4": (9, 0, 0),
    "stream": (0, 0, 0),
    "stream-digest": (0, 0, 0),
}


def descriptors(pkg, nb, nch, seed):
    ch = pkg.synth_descriptors(nb, nch=nch, seed=seed)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    return ch


# where the roll-over of channel i of the roll-over case falls (sample of the block), for a granule of two tiles:
#   tile r = 0, early: the anchor of tile r = 1 lies past chip 1024 (reduced, the next data bit in force)
#   tile r = 0, its last samples: the anchor of tile r = 1 lies in [1023, 1024) (not reduced: rendered as a tile with the roll-over due)
#   tile r = 1; and the same three in the block's second granule
ROLL_AT = (500, 1014, 1024 + 300, 2048 + 700, 2048 + 1015, 3072 + 100, 1023, 1024)


def rollover_case(pkg):
    nb, nch, nsamp = 3, 16, 5 * TILE + 100
    ch = descriptors(pkg, nb, nch, 0x7101)
    sc = ch["f_code"] * DELT
    for i in range(nch):
        at = ROLL_AT[i % len(ROLL_AT)]
        ch["code_phase"][:, i] = 1023.0 - sc[:, i] * (at + 0.5)  # chip 1023 is reached between samples `at` and `at` + 1
        if i < len(ROLL_AT):
            ch["icode"][:, i] = 19                                # the roll-over ends a data bit ...
            ch["dwrd"][:, i, :] = 0x2AAAAAAA if i % 2 == 0 else 0x15555555  # ... and the next one differs (alternating words)
            ch["ibit"][:, i] = 3 + i
        else:
            ch["icode"][:, i] = 4                                 # the same data bit goes on behind the roll-over
    # what the placements are for (the model's anchor of tile r = 1: the block's start phase 1024 steps on)
    anchor1 = ch["code_phase"] + 1024.0 * sc
    assert ((anchor1[:, 1] >= 1023.0) & (anchor1[:, 1] < 1024.0)).all() and (anchor1[:, 0] >= 1024.0).all()
    assert (anchor1[:, 2] < 1023.0).all() and (anchor1[:, 6] >= 1023.0).all() and (anchor1[:, 6] < 1024.0).all()
    return ch, nsamp, pkg.CHAIN_CARRIER


def carrier_case(pkg, nch):
    nb, nsamp = 3, 6 * TILE + 333
    ch = descriptors(pkg, nb, nch, 0x7102 + nch)
    f = ch["f_carr"]
    f[:, 0] = 3000.0          # rising
    f[:, 1] = -3000.0         # falling: walked mirrored
    f[:, 2] = 0.0             # no Doppler at all: the phase stands
    if nch > 3:
        f[:, 3] = 4900.0      # 4900 / 25e6 * 512 * 15.5 = 1.56: two index changes in a run of 16 samples
        f[:, 4] = -4900.0
        f[:, 5] = -0.0
        ch["carr_phase"][:, 6] = 0.0   # a falling carrier on phase 0: mirrored it stands on 512, the one anchor tile 0 reduces
        f[:, 6] = -1200.0
    ch["f_code"] = 1.023e6 + f / 1540.0
    return ch, nsamp, pkg.CHAIN_CARRIER


def tiles_case(pkg, nsamp):
    return descriptors(pkg, 3, 16, 0x7100 + nsamp % 97), nsamp, pkg.CHAIN_CARRIER


def chunk_case(pkg):
    """the smallest batch whose tiles the host still hands out four at a time: nblocks * ceil(ntiles / 4) >= 256 CUs * 16
    wavefronts — 64 blocks of 256 tiles"""
    return descriptors(pkg, 64, 16, 0x7104), 256 * TILE, 0


def stream_blocks(pkg):
    return descriptors(pkg, 24, 16, 0x7105), 6 * TILE + 200, pkg.CHAIN_CARRIER


CASES = {
    "tiles-1024": lambda pkg: tiles_case(pkg, 1024),
    "tiles-3112": lambda pkg: tiles_case(pkg, 3 * 1024 + 40),
    "tiles-4096": lambda pkg: tiles_case(pkg, 4 * 1024),
    "tiles-9232": lambda pkg: tiles_case(pkg, 9 * 1024 + 16),
    "rollover": rollover_case,
    "carriers-16": lambda pkg: carrier_case(pkg, 16),
    "carriers-3": lambda pkg: carrier_case(pkg, 3),
    "chunks-of-4": chunk_case,
    "stream": stream_blocks,
}

GRANULE_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package
pkg = load_package()
L = pkg.lib()
L.gpsbb_test_state_log2.argtypes = [ctypes.c_void_p]
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ev_tile_prologue_gpu as t
out = {}
with pkg.Synth(0) as s:
    for name, make in t.CASES.items():
        ch, nsamp, flags = make(pkg)
        b = s.batch(ch, t.DELT, nsamp, flags=flags)
        b.run(); s.sync()
        out[name] = [int(L.gpsbb_test_state_log2(b._b)), int(s.info(pkg.INFO_LAST_VARIANT)), int(s.info(pkg.INFO_PREPASS))]
        b.close()
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def granules(pkg):
    """every case's state granule, kernel and pre-pass as the experiments build (the same sources plus the test hooks) plans them:
    one child process for all of them"""
    env = dict(os.environ, GPSBB_PY_LIB="exp")
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + GRANULE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def counters(pkg, synth):
    synth.sync()
    hz = synth.hazards()
    return (synth.info(pkg.INFO_EXACT_RUNS), hz["itable_512"], hz["dwrd_oob"], synth.info(pkg.INFO_TILES_RENDERED))


def counted(pkg, synth, c0):
    c1 = counters(pkg, synth)
    return tuple(int(a - b) for a, b in zip(c1, c0))


def check_run(pkg, synth, granules, name, got, nb, nsamp):
    """the per-case asserts; got: the counters' growth over the breakpoint kernel's run(s)"""
    print("%s: exact runs %d, itable_512 %d, dwrd_oob %d, tiles %d" % ((name,) + got))
    assert granules[name.replace("-digest", "")] == [1, pkg.VARIANT_EV, 3], (name, granules)
    assert synth.info(pkg.INFO_LAST_KERNEL) == 2 and synth.info(pkg.INFO_LAST_VARIANT) == pkg.VARIANT_EV and synth.info(pkg.INFO_PREPASS) == 3
    assert got[3] == nb * ((nsamp + TILE - 1) // TILE), (name, got)


def check_parent(name, got):
    """the case's last assert: the counters of the parent commit's kernel for the same input"""
    assert got[:3] == tuple(PARENT[name]), (name, got, PARENT[name])


def render_batch(pkg, synth, ch, nsamp, flags):
    """-> IQ, end states, counters' growth, the blocks' device digests"""
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 0)
    c0 = counters(pkg, synth)
    b = synth.batch(ch, DELT, nsamp, flags=flags)
    b.run(); synth.sync()
    got = counted(pkg, synth, c0)
    iq, st = b.read()
    dig = synth.device_digest(b.device_iq(), ch.shape[0], nsamp)
    b.close()
    return iq, st, got, dig


def same_states(got, want, ch):
    act = ch["prn"] > 0
    return [f for f in STATE_FIELDS if got[f][act].tobytes() != want[f][act].tobytes()]


@pytest.fixture()
def fresh(pkg, synth):
    for opt in (pkg.OPT_SEED_WHERE, pkg.OPT_SYNTH_KERNEL, pkg.OPT_CHAIN_WHERE):
        synth.set_option(opt, 0)
    yield synth
    for opt in (pkg.OPT_SEED_WHERE, pkg.OPT_SYNTH_KERNEL, pkg.OPT_CHAIN_WHERE):
        synth.set_option(opt, 0)


@pytest.mark.parametrize("name", ["tiles-1024", "tiles-3112", "tiles-4096", "tiles-9232", "rollover", "carriers-16", "carriers-3"])
def test_against_the_oracle(pkg, fresh, oracle, granules, name):
    """Tile counts (a one-tile granule; an odd count with a partial last tile; even counts), roll-overs in tile r = 0 and r = 1 of a
    granule with a data bit that changes and one that does not (anchors in [1023, 1024) and past 1024), rising, falling, standing
    and fast carriers, 3 channels (6 chain lanes): three blocks each, so that helpers join and chunks are single tiles."""
    ch, nsamp, flags = CASES[name](pkg)
    want_iq, want_st, hz = oracle.fill_blocks(ch, DELT, nsamp, chain=bool(flags))
    iq, st, got, _ = render_batch(pkg, fresh, ch, nsamp, flags)
    check_run(pkg, fresh, granules, name, got, ch.shape[0], nsamp)
    bad = np.nonzero((iq != want_iq).any(axis=(1, 2)))[0]
    assert bad.size == 0, (name, "blocks whose IQ differs", bad.tolist(), "first sample", int(np.nonzero((iq[bad[0]] != want_iq[bad[0]]).any(axis=1))[0][0]))
    assert same_states(st, want_st, ch) == [], name
    assert (got[1], got[2]) == (int(hz["itable_512"]), int(hz["dwrd_oob"])), (name, got, hz)
    check_parent(name, got)


def test_chunks_of_four_tiles(pkg, fresh, oracle, granules):
    """64 blocks of 256 tiles: a wavefront takes four consecutive tiles — two whole granules — at a time.  Every block's digest
    against the per-sample kernel's, the first and the last block against the oracle."""
    s = fresh
    ch, nsamp, flags = CASES["chunks-of-4"](pkg)
    nb = ch.shape[0]
    iq, st, got, dig = render_batch(pkg, s, ch, nsamp, flags)
    check_run(pkg, s, granules, "chunks-of-4", got, nb, nsamp)
    s.set_option(pkg.OPT_SYNTH_KERNEL, 1)
    b = s.batch(ch, DELT, nsamp, flags=flags)
    b.run(); s.sync()
    assert s.info(pkg.INFO_LAST_KERNEL) == 1
    want_dig = s.device_digest(b.device_iq(), nb, nsamp)
    _, want_st = b.read(want_iq=False)
    b.close()
    s.set_option(pkg.OPT_SYNTH_KERNEL, 0)
    assert np.nonzero(dig != want_dig)[0].tolist() == []
    assert same_states(st, want_st, ch) == []
    for k in (0, nb - 1):
        o_iq, o_st, _ = oracle.fill_blocks(ch[k:k + 1], DELT, nsamp)
        assert (iq[k] == o_iq[0]).all() and same_states(st[k:k + 1], o_st, ch[k:k + 1]) == [], k
    check_parent("chunks-of-4", got)


@pytest.mark.parametrize("digest", [False, True])
def test_a_chained_stream_of_three_pushes(pkg, fresh, oracle, granules, digest):
    """Three pushes of 8 blocks through a device-only ring, the carrier chained across them; with GPSBB_PUSH_DIGEST the kernel that
    adds the digests up as it renders (k_synth_ev_digest) has the same body: the popped digests are device_digest of the slots."""
    s = fresh
    ch, nsamp, flags = CASES["stream"](pkg)
    bps, npush = 8, 3
    want_iq, want_st, _ = oracle.fill_blocks(ch, DELT, nsamp, chain=True)
    c0 = counters(pkg, s)
    stq = s.stream(16, DELT, nsamp, bps, depth=3, flags=flags | pkg.STREAM_DEVICE_ONLY)
    for k in range(npush):
        stq.push(ch[k * bps:(k + 1) * bps], digest=digest)
    s.sync()
    got = counted(pkg, s, c0)
    for k in range(npush):
        if digest:
            ptr, es, dig = stq.pop_digest()
            assert (dig == s.device_digest(ptr, bps, nsamp)).all(), k
            assert (dig == pkg.block_digest_host(want_iq[k * bps:(k + 1) * bps])).all(), k
        else:
            ptr, es = stq.pop()
        assert (s.device_read(ptr, (bps, nsamp, 2)) == want_iq[k * bps:(k + 1) * bps]).all(), k
        assert same_states(es, want_st[k * bps:(k + 1) * bps], ch[k * bps:(k + 1) * bps]) == [], k
    stq.close()
    check_run(pkg, s, granules, "stream-digest" if digest else "stream", got, bps * npush, nsamp)
    check_parent("stream-digest" if digest else "stream", got)
