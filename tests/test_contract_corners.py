"""The CPU oracle against the reference's own sample loop at the corners of the descriptor contract (tests/contract_corners.py:
code rates on either side of every planner threshold, gains at the admission limit and at the contract's edge, peaks of
+-32766, every PRN), and against the committed fixture of the same table where the reference is absent.  CPU only."""
import hashlib
import os

import numpy as np
import pytest

import contract_corners as cc
import oracle_binding as ob
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "contract_corners.npz")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_inputs(c, iq):
    """conditions on the table itself: a failure here says the table is wrong, not the library"""
    ch, delt = c["ch"], 1.0 / c["fs"]
    act = ch["prn"] > 0
    assert (np.abs(ch["f_carr"][act] * delt) <= 0.125).all() and (ch["iword"] <= 58).all() and (np.abs(ch["gain"]) < 2.0 ** 21).all()
    if c["sc"] is not None:
        assert all(float(f) * delt == c["sc"] for f in ch["f_code"][act]), c["name"]
    if c["peak"] is None:
        return
    which, cp = c["peak"]
    i, q = iq[:, 0].astype(np.int32), iq[:, 1].astype(np.int32)
    if which == "P1":
        assert (i.min(), i.max(), q.min(), q.max()) == (-32766, 32766, -32766, 32766), c["name"]
    elif which == "P2":
        comp = i if cp in (0.0, 0.5) else q   # cos at 0 and 0.5, sin at 0.25 and 0.75
        bound = 32750 if cp in (0.0, 0.25) else 32620   # the tables' negative peak is -510
        assert comp.max() >= bound and comp.min() <= -bound, (c["name"], comp.min(), comp.max())
    else:
        assert which == "P3"   # over the limit: the reference's (short) cast wraps peaks of +-51200
        assert (i == 51200 - 65536).any() and (i == 65536 - 51200).any() and (q == 51200 - 65536).any(), c["name"]


def test_the_table_covers_the_contract(pkg):
    T = cc.table(pkg)
    assert {int(p) for c in T for p in c["ch"]["prn"]} >= set(range(1, 33))
    assert {c["variant"] for c in T} == {cc.SYNTH, cc.EV, cc.EV_DENSE, cc.PD_WIDE, cc.PD_NARROW, cc.EV_FIXED}
    assert min(int(c["ch"]["iword"].min()) for c in T) == 0 and max(int(c["ch"]["iword"].max()) for c in T) == 58
    assert len({c["name"] for c in T}) == len(T)
    # the four cases at the chip table's reach: code phases within 2^-10 chips below 1023 at the first sample of a later tile
    import ctypes as C
    wr = C.c_longlong(0)
    for c in T:
        if c["kind"] == "code" and any(r in c["name"] for r in cc.REACH):
            assert c["ch"]["code_phase"][0] == np.nextafter(1023.0, 0.0)
            for i, tile in ((2, 3), (5, 41)):
                x = pkg.exp_lib().gpsbb_test_code_jump(float(c["ch"]["code_phase"][i]), c["sc"], 1024 * tile, C.byref(wr))
                assert 1023.0 - 2.0 ** -10 < x < 1023.0, (c["name"], i, x)


@pytest.mark.skipif(not ob.have_ref(), reason="oracle/_ref not built (no /root/reference here)")
@pytest.mark.parametrize("kind", ["code", "mixed", "gain", "peak"])
def test_oracle_against_the_reference_loop_in_the_corners(oracle, pkg, kind):
    """Oracle.fill_blocks == the reference's verbatim loop, -O0 and -O2 (and its fixed-carrier build for the fixed cases), in IQ
    and end-state bytes; both hazard counters 0; the inputs reach what they claim (exact products, peaks)."""
    refs = {False: [ob.RefLoop(""), ob.RefLoop("_O2")], True: [ob.RefLoop("_fixed")]}
    ncases = 0
    for c in cc.table(pkg):
        if c["kind"] != kind:
            continue
        ncases += 1
        iq, st, hz = oracle.fill_blocks(c["ch"], 1.0 / c["fs"], c["nsamp"], fixed=c["fixed"])
        assert hz["itable_512"] == 0 and hz["dwrd_oob"] == 0, c["name"]
        for r in refs[c["fixed"]]:
            riq, rst = r.fill(c["ch"], 1.0 / c["fs"], c["nsamp"])
            assert (iq[0] == riq).all(), c["name"]
            assert st[0].tobytes() == rst.tobytes(), c["name"]
        check_inputs(c, iq[0])
    assert ncases >= 32


def test_oracle_reproduces_the_corner_fixture(oracle, pkg):
    """tests/golden/contract_corners.npz (made from the reference's loop by tests/golden/make_golden.py): the table built here is
    the table the fixture was made from, and the oracle renders every case to the reference's SHA-256 and end states."""
    T = cc.table(pkg)
    z = np.load(FIXTURE)
    assert [str(n) for n in z["names"]] == [c["name"] for c in T]
    want_st = z["end_state"].view(ob.STATE_DTYPE).reshape(len(T), 16)
    for k, c in enumerate(T):
        assert cc.fixture_descriptors(z, k).tobytes() == c["ch"].tobytes(), c["name"]
        assert (float(z["fs"][k]), int(z["nsamp"][k]), bool(z["fixed"][k]), int(z["variant"][k])) == \
            (c["fs"], c["nsamp"], c["fixed"], c["variant"]), c["name"]
        iq, st, hz = oracle.fill_blocks(c["ch"], 1.0 / c["fs"], c["nsamp"], fixed=c["fixed"])
        assert hz["itable_512"] == 0 and hz["dwrd_oob"] == 0, c["name"]
        assert sha(iq[0]) == str(z["iq_sha256"][k]), c["name"]
        assert st[0].tobytes() == want_st[k, :len(c["ch"])].tobytes(), c["name"]
        check_inputs(c, iq[0])
