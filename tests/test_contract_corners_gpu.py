"""Every corner of the descriptor contract (tests/contract_corners.py) through every synthesis path of the HIP library:
bit-exact IQ and end states against the CPU oracle, the IQ's SHA-256 against the fixture made from the reference's own loop,
and the kernel each case is rendered by against the column the table states for it."""
import hashlib
import math
import os

import numpy as np
import pytest

import contract_corners as cc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("carr_phase", "code_phase", "iword", "ibit", "icode", "dataBit", "codeCA")
MODES = ["default", "k_seed+auto", "host+auto", "laps+auto", "k_seed+per-sample"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(autouse=True, params=MODES)
def seed_mode(pkg, synth, request):
    """Five ways: no option set (the library's own choices), then the pre-pass forced — row walks, host threads, lap-parallel —
    with the kernel left to the library, and the row walks with k_synth forced."""
    if request.param != "default":
        where, kernel = request.param.split("+")
        synth.set_option(pkg.OPT_SEED_WHERE, {"k_seed": 1, "host": 2, "laps": 3}[where])
        synth.set_option(pkg.OPT_SYNTH_KERNEL, 1 if kernel == "per-sample" else 0)
    yield request.param
    synth.set_option(pkg.OPT_SEED_WHERE, 0)
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 0)


_renders = {}


def rendered(pkg, oracle, k, chain=False):
    """the oracle's render of case k (or of its 3-block chain), once per session"""
    key = (k, chain)
    if key not in _renders:
        c = cc.table(pkg)[k]
        ch = cc.redrawn_chain(c) if chain else c["ch"]
        iq, st, hz = oracle.fill_blocks(ch, 1.0 / c["fs"], c["nsamp"], chain=chain, fixed=c["fixed"])
        assert hz["itable_512"] == 0 and hz["dwrd_oob"] == 0, c["name"]
        _renders[key] = (ch, iq, st)
    return _renders[key]


def state_diffs(got, want, active):
    return [f for f in STATE_FIELDS if got[f][active].tobytes() != want[f][active].tobytes()]


def check_kernel(pkg, synth, mode, c, bad, what):
    """in the modes that leave the kernel to the library: the variant the table states; the lap-parallel pre-pass wherever it is
    asked for and a model kernel renders (no step of the table is below 2^-50)"""
    v = synth.info(pkg.INFO_LAST_VARIANT)
    if mode.endswith("per-sample"):
        if v != cc.SYNTH or synth.info(pkg.INFO_LAST_KERNEL) != 1:
            bad.append("%s %s: k_synth forced, variant %d" % (c["name"], what, v))
        return
    if v != c["variant"]:
        bad.append("%s %s: rendered by %s, the table says %s" % (c["name"], what, cc.VARIANT_NAMES.get(v, v), cc.VARIANT_NAMES[c["variant"]]))
    if synth.info(pkg.INFO_LAST_KERNEL) != (1 if c["variant"] == cc.SYNTH else 2):
        bad.append("%s %s: GPSBB_INFO_LAST_KERNEL %d" % (c["name"], what, synth.info(pkg.INFO_LAST_KERNEL)))
    if mode == "laps+auto" and c["variant"] in cc.MODEL_VARIANTS and synth.info(pkg.INFO_PREPASS) != 3:
        bad.append("%s %s: pre-pass %d, lap-parallel asked for" % (c["name"], what, synth.info(pkg.INFO_PREPASS)))


@pytest.mark.parametrize("kind", ["code", "mixed", "gain", "peak"])
def test_every_corner_on_every_path(pkg, synth, oracle, seed_mode, kind):
    """gpsbb_fill_block of every case (and a 3-block GPSBB_CHAIN_CARRIER batch of the mixed and peak cases): IQ and all seven
    end-state fields equal to the oracle's, the IQ's SHA-256 equal to the reference loop's (the fixture), no hazard counted, the
    kernel the table states, and exactly ceil(nsamp / 1024) tiles per block on the model kernels."""
    T = cc.table(pkg)
    z = np.load(os.path.join(GOLDEN, "contract_corners.npz"))
    assert [str(n) for n in z["names"]] == [c["name"] for c in T]
    synth.hazards(reset=True)
    bad = []
    ncases = 0
    for k, c in enumerate(T):
        if c["kind"] != kind:
            continue
        ncases += 1
        delt, nsamp = 1.0 / c["fs"], c["nsamp"]
        flags = pkg.FIXED_CARRIER if c["fixed"] else 0
        ch, want_iq, want_st = rendered(pkg, oracle, k)
        model = c["variant"] in cc.MODEL_VARIANTS and not seed_mode.endswith("per-sample")
        tiles0 = synth.info(pkg.INFO_TILES_RENDERED)
        iq, st = synth.fill_block(ch, delt, nsamp, flags=flags)
        tiles = synth.info(pkg.INFO_TILES_RENDERED) - tiles0
        check_kernel(pkg, synth, seed_mode, c, bad, "fill")
        if not (iq == want_iq[0]).all():
            w = np.nonzero((iq != want_iq[0]).any(axis=1))[0]
            bad.append("%s: %d samples differ from the oracle, first %d" % (c["name"], w.size, w[0]))
        if sha(iq) != str(z["iq_sha256"][k]):
            bad.append("%s: SHA-256 of the IQ is not the reference loop's" % c["name"])
        d = state_diffs(st, want_st[0], ch["prn"] > 0)
        if d:
            bad.append("%s: end state %s" % (c["name"], d))
        if tiles != (math.ceil(nsamp / 1024) if model else 0):
            bad.append("%s: %d tiles rendered by the model kernels" % (c["name"], tiles))
        if kind in ("mixed", "peak"):
            ch3, want_iq3, want_st3 = rendered(pkg, oracle, k, chain=True)
            tiles0 = synth.info(pkg.INFO_TILES_RENDERED)
            b = synth.batch(ch3, delt, nsamp, flags=flags | pkg.CHAIN_CARRIER)
            b.run()
            synth.sync()
            iq3, st3 = b.read()
            b.close()
            tiles = synth.info(pkg.INFO_TILES_RENDERED) - tiles0
            check_kernel(pkg, synth, seed_mode, c, bad, "chain")
            if not (iq3 == want_iq3).all():
                bad.append("%s chain: blocks %s differ from the oracle" % (c["name"], np.nonzero((iq3 != want_iq3).any(axis=(1, 2)))[0].tolist()))
            for blk in range(3):
                d = state_diffs(st3[blk], want_st3[blk], ch3["prn"][blk] > 0)
                if d:
                    bad.append("%s chain block %d: end state %s" % (c["name"], blk, d))
            if tiles != (3 * math.ceil(nsamp / 1024) if model else 0):
                bad.append("%s chain: %d tiles rendered by the model kernels" % (c["name"], tiles))
    hz = synth.hazards(reset=True)
    assert ncases >= 32
    assert not bad, "%d findings in %d cases:\n%s" % (len(bad), ncases, "\n".join(bad[:60]))
    assert hz == {"itable_512": 0, "dwrd_oob": 0}


def test_peaks_through_the_packed_formats(pkg, synth, oracle):
    """Components of +-32766 (and the wrapped +-51200) through GPSBB_OUT_SC8(0), _SC8(8) and _SC1 against pack_iq() of the
    oracle's IQ, and the SC8 clip counter against a count in numpy."""
    bad = []
    for k, c in enumerate(cc.table(pkg)):
        if c["kind"] != "peak":
            continue
        delt = 1.0 / c["fs"]
        flags = pkg.FIXED_CARRIER if c["fixed"] else 0
        ch, want_iq, _ = rendered(pkg, oracle, k)
        for fmt, nsamp in ((pkg.OUT_SC8(0), c["nsamp"]), (pkg.OUT_SC8(8), c["nsamp"]), (pkg.OUT_SC1, c["nsamp"] // 4 * 4)):
            want = want_iq[0, :nsamp]   # (a shorter block is a prefix of the longer one)
            clip0 = synth.info(pkg.INFO_SC8_CLIPPED)
            got, _ = synth.fill_block(ch, delt, nsamp, flags=flags, fmt=fmt)
            clipped = synth.info(pkg.INFO_SC8_CLIPPED) - clip0
            if not (got == pkg.pack_iq(want, fmt)).all():
                bad.append("%s fmt 0x%x: packed bytes differ" % (c["name"], fmt))
            if fmt != pkg.OUT_SC1:
                s = want.astype(np.int32) >> ((fmt & pkg.OUT_SHIFT_MASK) >> 12)
                if clipped != int(np.count_nonzero((s < -128) | (s > 127))):
                    bad.append("%s fmt 0x%x: %d components counted as clipped" % (c["name"], fmt, clipped))
            elif clipped:
                bad.append("%s SC1: clip counter moved" % c["name"])
    assert not bad, "\n".join(bad[:40])


def test_contract_edges_are_refused(pkg, synth, oracle):
    """One step outside the contract is GPSBB_E_BADCHAN, and the handle renders the next block as if nothing had happened."""
    fs, nsamp = 2.6e6, 20001
    good = cc.base(12, 4242, prn0=20)
    want_iq, want_st, _ = oracle.fill_blocks(good, 1.0 / fs, nsamp)

    def edit(field, value, i=3):
        ch = good.copy()
        ch[field][i] = value
        return ch

    edges = {
        "sc above 1.5": edit("f_code", cc.f_code_for(math.nextafter(1.5, 2.0), fs)),
        "f_code = 0": edit("f_code", 0.0),
        "-f_code": edit("f_code", -good["f_code"][3]),
        "gain = 2^21": edit("gain", 2.0 ** 21),
        "gain = -2^21": edit("gain", -2.0 ** 21),
        "iword = 60": edit("iword", 60),
        "PRN 33": edit("prn", 33),
    }
    for name, ch in edges.items():
        with pytest.raises(pkg.GpsbbError) as e:
            synth.fill_block(ch, 1.0 / fs, nsamp)
        assert e.value.rc == -2, name
        with pytest.raises(pkg.GpsbbError) as e:
            synth.batch(np.stack([good, ch]), 1.0 / fs, nsamp)
        assert e.value.rc == -2, name
        iq, st = synth.fill_block(good, 1.0 / fs, nsamp)
        assert (iq == want_iq[0]).all() and not state_diffs(st, want_st[0], good["prn"] > 0), name
    # ... and the contract's own last values are taken
    for field, value in (("f_code", cc.f_code_for(1.5, fs)), ("gain", math.nextafter(2.0 ** 21, 0.0)), ("iword", 59), ("prn", 32)):
        ch = edit(field, value)
        w_iq, w_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
        iq, st = synth.fill_block(ch, 1.0 / fs, nsamp)
        assert (iq == w_iq[0]).all() and not state_diffs(st, w_st[0], ch["prn"] > 0), field
    synth.hazards(reset=True)


@pytest.mark.parametrize("name", ["mixed code rates 2.5e+07 16", "code 0.5 2.6e+06 12"])
def test_corner_code_rates_through_a_chained_ring(pkg, synth, oracle, seed_mode, name):
    """The push path plans on its own: three pushes of two blocks through a host-gather ring, chained, against the oracle's
    chained render."""
    T = cc.table(pkg)
    c = [c for c in T if c["name"] == name][0]
    ch = cc.redrawn_chain(c, nblocks=6)
    delt, nsamp = 1.0 / c["fs"], c["nsamp"]
    want_iq, want_st, hz = oracle.fill_blocks(ch, delt, nsamp, chain=True)
    assert hz["itable_512"] == 0 and hz["dwrd_oob"] == 0
    s = synth.stream(len(c["ch"]), delt, nsamp, 2, depth=3, flags=pkg.CHAIN_CARRIER)
    bad = []
    for p in range(3):
        s.push(ch[2 * p:2 * p + 2])
        check_kernel(pkg, synth, seed_mode, c, bad, "push %d" % p)
    got = [s.pop() for _ in range(3)]
    s.close()
    assert not bad, "\n".join(bad)
    assert (np.concatenate([g[0] for g in got]) == want_iq).all()
    st = np.concatenate([g[1] for g in got])
    for blk in range(6):
        assert not state_diffs(st[blk], want_st[blk], ch["prn"][blk] > 0), blk
    assert synth.hazards(reset=True) == {"itable_512": 0, "dwrd_oob": 0}
