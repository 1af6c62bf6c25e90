"""What a device-only ring's pop hands out as `ends` is the states of the push it pops, never a neighbour's.  The slot's pinned
end states are written by a small kernel (k_end_states_to_host) from the table set the push's pre-pass filled; pre-passes run
ahead, beside the synthesis of the pushes before, and slots and table sets are reused — so whichever stream carries that copy
(DESIGN.md 4.1 and the appendix: behind the synthesis, or behind the pre-pass) it has to read the right set, after the repair
kernel, into the right slot.  A chained ring of depth 2 fed five pushes, so that both slots are written again while their
neighbour is in flight, against the oracle's chained states: by the lap-parallel pre-pass, by the row walks, and with the
experiments build's GPSBB_LAP_JITTER, where k_lap_repair rewrites states behind pass 2.

Run as a script (the jitter case: the library is chosen when the package is imported) it prints the links that did not hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA")
NCH, FS, NSAMP, BPS, PUSHES, DEPTH = 16, 25e6, 5000, 2, 5, 2
# the jitter case's Doppler range: at the +-5 kHz of the other cases these ten short blocks hold so few laps that no link breaks
# (measured: 0 at 5 and 50 kHz, 1 at 500 kHz) and the repair kernel would have nothing to rewrite
JITTER_DOPPLER = 500000.0

pytestmark = pytest.mark.gpu


def ring_against_oracle(pkg, synth, oracle, where, max_doppler=5000.0):
    """five pushes through a ring of two slots; every pop's seven fields and IQ against the oracle's blocks of that push"""
    ch = pkg.synth_descriptors(PUSHES * BPS, nch=NCH, seed=0xE5D, max_doppler=max_doppler)
    want_iq, want_st, _ = oracle.fill_blocks(ch, 1 / FS, NSAMP, chain=True)
    synth.set_option(pkg.OPT_SEED_WHERE, where)
    try:
        ring = synth.stream(NCH, 1 / FS, NSAMP, BPS, depth=DEPTH, flags=pkg.CHAIN_CARRIER | pkg.STREAM_DEVICE_ONLY)
        done = 0

        def pop_one():
            nonlocal done
            p, st = ring.pop()
            lo, hi = done * BPS, (done + 1) * BPS
            for f in FIELDS:
                assert st[f].tobytes() == want_st[f][lo:hi].tobytes(), "push %d: %s is not that push's (seed where %d)" % (done, f, where)
            assert (synth.device_read(p, (BPS, NSAMP, 2)) == want_iq[lo:hi]).all(), "push %d: IQ" % done
            done += 1

        for k in range(PUSHES):
            if ring.pending == DEPTH:
                pop_one()
            ring.push(ch[k * BPS:(k + 1) * BPS])
            assert synth.info(pkg.INFO_PREPASS) == (3 if where in (0, 3) else 1)
        while ring.pending:
            pop_one()
        ring.close()
        assert done == PUSHES
    finally:
        synth.set_option(pkg.OPT_SEED_WHERE, 0)


@pytest.mark.parametrize("where", [0, 1], ids=["laps", "row-walks"])
def test_every_pop_has_its_own_pushs_end_states(pkg, synth, oracle, where):
    ring_against_oracle(pkg, synth, oracle, where)


def test_the_repair_kernel_is_done_before_they_leave(pkg):
    if not os.path.exists(pkg.EXP_LIB_PATH):
        pytest.skip("no experiments build")
    env = dict(os.environ, GPSBB_PY_LIB="exp", GPSBB_LAP_JITTER="4000000000")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(JITTER_DOPPLER)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "end states ok" in r.stdout
    assert int(r.stdout.split("links that did not hold:")[1].split()[0]) >= 1, r.stdout[-600:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    from conftest import load_package
    import oracle_binding as ob
    pkg_ = load_package()
    with pkg_.Synth(0) as s_:
        r0 = s_.info(pkg_.INFO_CHAIN_REPAIRS)
        ring_against_oracle(pkg_, s_, ob.Oracle(), 3, float(sys.argv[1]) if len(sys.argv) > 1 else 5000.0)
        print("end states ok; links that did not hold: %d" % (s_.info(pkg_.INFO_CHAIN_REPAIRS) - r0))
