"""gpsbb_device_track on the GPU (k_track): every comparison is == on every field of every record, every count and every returned
state against track_host fed with view_host's output (tools/track_check.py), on the smallest shapes at which the kernel can go
wrong — a ragged third pass of the lanes, a buffer that ends on an epoch's last sample, every view plain and impaired, the
accumulators at their largest, the clamps, a call split in three — every refusal; and end to end: six rendered satellites
acquired, tracked, and their data bits read back by calls that are told nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import track_check as tc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1
LEN = 1023 << 32
CMAX = (1 << 47) - 1


def clips(pkg, synth):
    return synth.info(pkg.INFO_SC8_CLIPPED), synth.info(pkg.INFO_NOISE_CLIPPED)


def test_1_lane_and_wave_map(pkg, synth):
    """Random full-range int16 IQ (not a render) with +-32767 and -32768 in it, code_nom = 3 << 31 so that N is 682 or 683 — two
    full passes of the 256 lanes and a ragged third —, PRNs {1, 7, 17, 32} with different steps, phases and first samples,
    nfll = 6 and 12 epochs: both discriminators run."""
    iq, cfg, st = tc.lane_map_case(pkg)
    assert {32767, -32767, -32768} <= set(iq[:, 0].tolist()) and {32767, -32768} <= set(iq[:, 1].tolist())
    assert st["prn"].tolist() == [1, 7, 17, 32] and (cfg.code_nom, cfg.nfll, cfg.max_epochs) == (3 << 31, 6, 12)
    got = tc.on_device(pkg, synth, iq, cfg, st)
    want = tc.mirror(pkg, iq, cfg, st)
    bad = tc.compare(got, want)
    assert not bad, "\n".join(bad)
    for r in got[1]:
        assert r.size == 12 and r["mode"].tolist() == [0] * 6 + [1] * 6 and 606 <= r["N"][1:].min() and r["N"].max() <= 780
        assert r["e_c"][1:].any() and r["e_d"].any() and r["p_i"].all()
    assert got[1][0]["N"][0] == 682 and got[1][2]["N"][0] == 1   # (channel 2 starts one unit short of its code's end)


def test_2_ends(pkg, synth):
    """nsamp exactly at the end of channel 0's fifth epoch: five records; one short: four, and that channel's state is the one
    after four epochs.  Five spare samples of 0x7fff behind the buffer, told to the call and not told: no sum sees them.
    max_epochs smaller than what fits."""
    iq, cfg, st = tc.ends_case(pkg)
    s5, _ = pkg.track_host(pkg.view_host(iq), cfg.copy(max_epochs=5), st)
    s4, _ = pkg.track_host(pkg.view_host(iq), cfg.copy(max_epochs=4), st)
    n = int(s5["n0"][0])
    bad = []
    want = tc.mirror(pkg, iq, cfg, st, nsamp=n)
    got = tc.on_device(pkg, synth, iq[:n], cfg, st)
    bad += tc.compare(got, want, "exact length")
    assert got[1][0].size == 5 and got[0][0].tobytes() == s5[0].tobytes()
    short = tc.on_device(pkg, synth, iq[:n - 1], cfg, st)
    bad += tc.compare(short, tc.mirror(pkg, iq, cfg, st, nsamp=n - 1), "one short")
    assert short[1][0].size == 4 and short[0][0].tobytes() == s4[0].tobytes()
    iq5 = np.concatenate([iq[:n], np.full((5, 2), 0x7FFF, np.int16)])
    bad += tc.compare(tc.on_device(pkg, synth, iq5, cfg, st), want, "5 spare samples, nsamp + 5")
    bad += tc.compare(tc.on_device(pkg, synth, iq5, cfg, st, nsamp=n), want, "5 spare samples, nsamp")
    few = cfg.copy(max_epochs=3)
    got3 = tc.on_device(pkg, synth, iq, few, st)
    bad += tc.compare(got3, tc.mirror(pkg, iq, few, st), "max_epochs 3")
    assert [r.size for r in got3[1]] == [3, 3]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("impair", ["plain", "noise", "noise+chirp", "chirp"])
@pytest.mark.parametrize("name", ["sc16", "sc8", "sc1"])
def test_3_views(pkg, synth, name, impair):
    """Eight epochs of two channels in SC16, SC8(5) and SC1: plain, with a gpsbb_noise_t whose sample0 lies above 2^32, with noise
    and a chirp, and with the chirp alone.  The handle's clip counters do not move."""
    view = {"sc16": pkg.OUT_SC16, "sc8": pkg.OUT_SC8(5), "sc1": pkg.OUT_SC1}[name]
    iq, cfg, st = tc.views_case(pkg)
    delt = 1.0 / tc.FS
    nz = pkg._as_noise(tc.NOISE) if "noise" in impair else None
    assert tc.NOISE["sample0"] > 1 << 32
    js = None
    if "chirp" in impair:
        js = pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -0.2 * tc.FS, 0.27 * tc.FS, 301 * delt, delt=delt)], tc.NOISE["shift"],
                           tc.NOISE["sample0"])
    before = clips(pkg, synth)
    got = tc.on_device(pkg, synth, iq, cfg, st, view, nz, js)
    bad = tc.compare(got, tc.mirror(pkg, iq, cfg, st, view, nz, js), "%s %s" % (name, impair))
    assert not bad, "\n".join(bad)
    assert clips(pkg, synth) == before and [r.size for r in got[1]] == [8, 8]
    if impair != "plain":   # the impairment is really in the view
        assert (pkg.view_host(iq, view, nz, interf=js) != pkg.view_host(iq, view)).any()


def test_4_accumulator_range(pkg, synth):
    """Every component -32768, the carrier at rest at table index 64, the smallest legal code_nom: two epochs of 917 505 samples,
    every lane's partial sums at their largest.  == the mirror, and in closed form: y is one number for every sample, so
    P = (the sum of the epoch's chips) * y."""
    iq, cfg, st = tc.range_case(pkg)
    assert cfg.code_nom == tc.smallest_code_nom()
    got = tc.on_device(pkg, synth, iq, cfg, st)
    bad = tc.compare(got, tc.mirror(pkg, iq, cfg, st))
    assert not bad, "\n".join(bad)
    r = got[1][0]
    assert r.size == 2 and r["N"][0] == 917505 and r["N"][1] >= 917504
    sin512, cos512 = pkg.sincos_tables()
    c, s = int(cos512[64]), int(sin512[64])
    yi, yq = -32768 * c + -32768 * s, -32768 * c - -32768 * s
    x = 2 * pkg.codegen(13).astype(np.int64) - 1
    for k in range(2):
        j = np.arange(int(r["N"][k]), dtype=np.uint64)
        chips = int(x[((np.uint64(r["code_phase"][k]) + np.uint64(cfg.code_nom) * j) >> np.uint64(32)).astype(np.int64)].sum())
        assert (int(r["p_i"][k]), int(r["p_q"][k])) == (chips * yi, chips * yq) and chips != 0
        assert int(r["q"][k]) > 0 and abs(yi) > 1 << 23


def test_5_clamps(pkg, synth):
    """kf, kp1 and kd1 at 2^31 - 1 on random data, 10 epochs: == the mirror, and the records show carr_step at +(2^47 - 1) and at
    -(2^47 - 1) and cs at both ends of its clamp (tests/test_track.py checks on the CPU that this data reaches them)."""
    iq, cfg, st = tc.clamps_case(pkg)
    got = tc.on_device(pkg, synth, iq, cfg, st)
    bad = tc.compare(got, tc.mirror(pkg, iq, cfg, st))
    assert not bad, "\n".join(bad)
    s, recs = got
    steps = [int(v) for r in recs for v in r["carr_step"]] + [int(v) for v in s["carr_step"]]
    cs = [v for c in range(2) for v in tc.records_cs(recs[c], s[c])]
    nom = cfg.code_nom
    assert CMAX in steps and -CMAX in steps and nom - nom // 8 in cs and nom + nom // 8 in cs


def test_6_resume(pkg, synth):
    """One call of 40 epochs == calls of 13, 1 and 26 with the returned states, with noise on; two channels with the same PRN in
    the same state give the same records."""
    iq, cfg, st = tc.resume_case(pkg)
    whole = tc.on_device(pkg, synth, iq, cfg, st, 0, tc.NOISE)
    bad = tc.compare(whole, tc.mirror(pkg, iq, cfg, st, 0, tc.NOISE), "whole")
    assert [r.size for r in whole[1]] == [40, 40, 40] and whole[1][0].tobytes() == whole[1][1].tobytes()
    assert whole[0][0].tobytes() == whole[0][1].tobytes()
    s, parts = st, [[], [], []]
    for n in (13, 1, 26):
        s, recs = tc.on_device(pkg, synth, iq, cfg.copy(max_epochs=n), s, 0, tc.NOISE)
        for c in range(3):
            assert recs[c].size == n
            parts[c].append(recs[c])
    bad += tc.compare((s, [np.concatenate(p) for p in parts]), whole, "13 + 1 + 26")
    assert not bad, "\n".join(bad)


def test_7_refusals(pkg, synth, oracle):
    """Every GPSBB_E_BADARG of the definition and the served neighbour of each; after every refusal the handle still renders a block
    bit-exactly, and states, records and counts are as they were."""
    import torch
    L = pkg.lib()
    n = 4000
    t = torch.zeros((n + 8, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    good = tc.make_cfg(pkg, max_epochs=2)
    st0 = tc.make_states(pkg, [dict(prn=1), dict(prn=32, epoch=3, prev_i=5, prev_q=-7)])
    ch = pkg.synth_descriptors(1, nch=4, seed=31)[0]
    delt = 1.0 / tc.FS
    want_iq = oracle.fill_blocks(ch[None, :], delt, 1500)[0][0]
    recs = np.zeros((2, 2), pkg.TRK_EPOCH_DTYPE)
    counts = np.full(2, -5, np.int32)

    def rc(cfg=good, ptr=t.data_ptr(), nsamp=n, view=0, nz=None, js=None, st=st0, nch=None, out=recs, cnt=counts, null_cfg=False, null_st=False, h=None):
        s = np.array(st, pkg.TRK_STATE_DTYPE)
        keep = s.tobytes()
        r = L.gpsbb_device_track(synth._h if h is None else h, C.c_void_p(ptr) if ptr else None, nsamp, view, None if nz is None else C.byref(nz),
                                 None if js is None else C.byref(js), None if null_cfg else C.byref(cfg), None if null_st else s.ctypes.data,
                                 s.size if nch is None else nch, None if out is None else out.ctypes.data, None if cnt is None else cnt.ctypes.data)
        if r != 0:
            assert s.tobytes() == keep and not recs.view(np.uint8).any() and (counts == -5).all()
        return r

    def still_renders():
        iq, _ = synth.fill_block(ch, delt, 1500)
        assert (iq == want_iq).all()

    def served(**kw):
        r = rc(**kw)
        recs[:] = 0
        counts[:] = -5
        return r == 0

    def one(**f):
        s = st0.copy()
        for k, v in f.items():
            s[k][0] = v
        return s

    assert served()
    still_renders()
    nz_ok = pkg.Noise(1, 5, 100.0, 1, 0)
    cw = pkg.interf_make(pkg.INTERF_CW, 0.0, 1000.0, delt=delt)
    nom_min = tc.smallest_code_nom()
    cases = [("d_iq NULL", dict(ptr=0)), ("cfg NULL", dict(null_cfg=True)), ("states NULL", dict(null_st=True)), ("epochs NULL", dict(out=None)),
             ("counts NULL", dict(cnt=None)), ("d_iq misaligned", dict(ptr=t.data_ptr() + 2)), ("nsamp 0", dict(nsamp=0)), ("nsamp < 0", dict(nsamp=-1)),
             ("nch 0", dict(nch=0)), ("nch 33", dict(nch=33)), ("nch < 0", dict(nch=-1)),
             ("code_nom 0", dict(cfg=good.copy(code_nom=0))), ("code_nom above 1.5 chips", dict(cfg=good.copy(code_nom=(3 << 31) + 1))),
             ("code_nom too small for N <= 2^20", dict(cfg=good.copy(code_nom=nom_min - 1))), ("spacing 0", dict(cfg=good.copy(spacing=0))),
             ("nfll < 0", dict(cfg=good.copy(nfll=-1))), ("max_epochs 0", dict(cfg=good.copy(max_epochs=0))),
             ("max_epochs 2^20 + 1", dict(cfg=good.copy(max_epochs=(1 << 20) + 1))),
             ("prn 0", dict(st=one(prn=0))), ("prn 33", dict(st=one(prn=33))), ("epoch < 0", dict(st=one(epoch=-1))), ("n0 < 0", dict(st=one(n0=-1))),
             ("n0 > nsamp", dict(st=one(n0=n + 1))), ("code_phase LEN", dict(st=one(code_phase=LEN))),
             ("carr_int 2^47", dict(st=one(carr_int=1 << 47))), ("carr_int -2^47", dict(st=one(carr_int=-(1 << 47)))),
             ("carr_step 2^47", dict(st=one(carr_step=1 << 47))), ("carr_step -2^47", dict(st=one(carr_step=-(1 << 47)))),
             ("code_int beyond its clamp", dict(st=one(code_int=(1 << 56) + 1))), ("code_adj beyond what step 6 leaves", dict(st=one(code_adj=-(1 << 49) - 1))),
             ("a previous prompt of 22 bits", dict(st=one(epoch=1, prev_q=1 << 20))),
             ("a bad state in the last channel", dict(st=np.concatenate([st0, one(prn=40)[:1]]))),
             ("unknown format", dict(view=3 << 8)), ("a shift on SC16", dict(view=0x1000)), ("bits below the format", dict(view=1)),
             ("bits above the shift", dict(view=1 << 16)),
             ("noise sigma 0", dict(nz=pkg.Noise(1, 0, 0.0, 0, 0))), ("noise shift 8", dict(nz=pkg.Noise(1, 0, 100.0, 8, 0))),
             ("a set of 5 emitters", dict(js=_set_n(pkg, cw, 5))), ("a set's shift 8", dict(js=pkg.InterfSet([cw], 8, 0))),
             ("noise and set apart in sample0", dict(nz=nz_ok, js=pkg.InterfSet([cw], 1, 6))),
             ("noise and set apart in shift", dict(nz=nz_ok, js=pkg.InterfSet([cw], 2, 5)))]
    for what, kw in cases:
        assert rc(**kw) == BADARG, what
        still_renders()
    assert L.gpsbb_device_track(None, C.c_void_p(t.data_ptr()), n, 0, None, None, C.byref(good), st0.copy().ctypes.data, 2, recs.ctypes.data,
                                counts.ctypes.data) == BADARG
    # the neighbours of the refusals are served
    assert served(nsamp=1) and served(nch=1) and served(cfg=good.copy(code_nom=3 << 31)) and served(cfg=good.copy(spacing=1))
    assert served(cfg=good.copy(spacing=(1 << 32) - 1, nfll=0, max_epochs=1)) and served(st=one(n0=n)) and served(st=one(code_phase=LEN - 1))
    assert served(st=one(carr_int=CMAX, carr_step=-CMAX)) and served(st=one(code_int=1 << 56, code_adj=-(1 << 49)))
    assert served(st=one(epoch=1, prev_q=(1 << 20) - 1, prev_i=-(1 << 20))) and served(st=one(epoch=0, prev_q=1 << 40))
    assert served(nz=nz_ok, js=pkg.InterfSet([cw], 1, 5)) and served(view=pkg.OUT_SC8(15)) and served(view=pkg.OUT_SC1)
    # ... the smallest code_nom with room for one of its epochs, and 32 channels of one PRN
    big = torch.zeros(((1 << 20) + 8, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert served(cfg=good.copy(code_nom=nom_min, max_epochs=1), ptr=big.data_ptr(), nsamp=1 << 20, st=st0[:1], out=recs[:1], cnt=counts[:1])
    many = np.zeros((32, 2), pkg.TRK_EPOCH_DTYPE)
    cnt32 = np.zeros(32, np.int32)
    assert rc(st=np.repeat(st0[:1], 32), out=many, cnt=cnt32) == 0 and (cnt32 == 2).all() and all(many[c].tobytes() == many[0].tobytes() for c in range(32))
    still_renders()


def _set_n(pkg, e, n):
    js = pkg.InterfSet([e], 0, 0)
    js.n = n
    return js


@pytest.mark.parametrize("name", ["sc16", "sc1"])
def test_8_end_to_end(pkg, synth, name):
    """synth_descriptors(1, nch=6, seed=0xACC) rendered by the library at 2.6 MS/s in one block of 1 300 000 samples (the render
    equals the oracle's by the project's contract).  gpsbb_device_acquire on its first 7800 samples with acq_make(delt, -5000,
    250, 41, 1e-3, 0, 2, view) and all 32 PRNs, trk_seed from acq_best, gpsbb_device_track with trk_make's constants, trk_bitsync
    (skip = 150) and trk_bits.  Per PRN: the carrier within 1 Hz of f_carr over the last 50 epochs, one non-zero histogram bin at
    (-(icode + 1)) mod 20, the 16 or 17 bits all equal or all opposite to the descriptor's.  The records of PRNs 1 and 4 (the
    weakest: gain 0.34) == the mirror's."""
    view = {"sc16": pkg.OUT_SC16, "sc1": pkg.OUT_SC1}[name]
    ch = tc.e2e_descriptors(pkg)
    acq = tc.e2e_acq_cfg(pkg, view)
    trk = tc.e2e_trk_cfg(pkg)
    assert (acq.ncoh, acq.nlags, acq.nnc, acq.nbins, acq.prn_mask) == (2600, 2600, 2, 41, 0xFFFFFFFF)
    b = synth.batch(ch, 1.0 / tc.FS, tc.E2E_NSAMP)
    try:
        b.run()
        synth.sync()
        rows = synth.device_acquire(b.device_iq(), tc.E2E_ACQ_NSAMP, acq, view)
        st = tc.e2e_seeds(pkg, rows, acq)
        after, recs = synth.device_track(b.device_iq(), tc.E2E_NSAMP, trk, st, view)
        iq, _ = b.read()
    finally:
        b.close()
    bad, (min_pi, max_pq) = tc.e2e_findings(pkg, ch, recs)
    print("%s: min |P.i| %.3g, max |P.q| %.3g after epoch %d; records %s" % (name, min_pi, max_pq, tc.E2E_SKIP, [r.size for r in recs]))
    assert not bad, "\n".join(bad)
    two = [0, 3]
    assert abs(float(ch[0, 3]["gain"]) - 0.34) < 0.01 and st["prn"][two].tolist() == [1, 4]
    want = pkg.track_host(pkg.view_host(iq[0], view), trk, st[two])
    bad = tc.compare((after[two], [recs[c] for c in two]), want, "PRNs 1 and 4")
    assert not bad, "\n".join(bad)
