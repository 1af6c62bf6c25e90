"""gpsbb_batch_despread_lags on the GPU (k_despread_lags): every comparison is == on int64 against despread_lags_host fed with
the CPU oracle's replicas (tools/despread_lags_check.py), on the smallest shapes at which the kernel can go wrong — a ragged
last tile, two chained blocks, a state per tile and per two tiles, a block shorter than a wavefront — in every view, with the
exact path made common, and end to end from a front end with echoes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import contract_corners as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_lags_check as dlc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG, STATE = -1, -7
LAGS = dlc.LAGS


@pytest.fixture
def default_options(pkg, synth):
    yield
    synth.set_option(pkg.OPT_SEED_WHERE, 0)
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 0)


_cases = {}


def case(pkg, oracle, name):
    """one of tools/despread_lags_check.py's cases with the oracle's chained render and replicas, once per session"""
    if not _cases:
        _cases.update(dlc.cases(pkg))
    return dlc.with_oracle(oracle, _cases[name])


def run_batch(pkg, synth, g):
    b = synth.batch(g["ch"], g["delt"], g["nsamp"], flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    return b


@pytest.mark.parametrize("where", [0, 1])
def test_pd_twelve_slots_one_prn_twice(pkg, synth, oracle, default_options, where):
    """2.6 MS/s, 12 slots — one idle, one PRN in two of them (a direct channel and its echo from gpsfe) — nsamp = 3 * 1024 + 37, 2
    chained blocks, k_synth_pd; lags at both ends of the range, unsorted; seg_tiles 1, 2 and longer than the block; behind the
    lap pre-pass and behind the row walks."""
    g = case(pkg, oracle, "pd")
    assert g["ch"].shape == (2, 12) and (g["ch"]["prn"][:, 4] == 0).all() and (g["ch"]["prn"][:, 0] == g["ch"]["prn"][:, 11]).all()
    synth.set_option(pkg.OPT_SEED_WHERE, where)
    b = run_batch(pkg, synth, g)
    variant = synth.info(pkg.INFO_LAST_VARIANT)
    iq, _ = b.read()
    bad = dlc.check_batch(pkg, b, g["iq"], g["rep"], (1, 2, 9))
    got = b.despread_lags(LAGS, seg_tiles=9)
    b.close()
    assert variant == dlc.dc.PD_WIDE
    assert (iq == g["iq"]).all()   # two channels with one PRN in a block render like any two
    assert not bad, "\n".join(bad)
    assert got.shape == (2, 12, 1, 8, 2) and not got[:, 4].any()


@pytest.mark.parametrize("name", ["ev", "ev_odd"])
def test_ev_a_state_per_two_tiles(pkg, synth, oracle, default_options, name):
    """25 MS/s, 16 channels behind the lap pre-pass, one state per two tiles, the same lags.  nsamp = 5 * 1024 + 37 is six tiles,
    the last 37 samples long; nsamp = 4 * 1024 + 37 is five, so the last state serves one tile.  The launcher hands a batch
    this small its tiles one at a time, so no chunk edge falls inside either: test_chunks_of_four_tiles_on_a_large_batch has
    those."""
    g = case(pkg, oracle, name)
    assert -(-g["nsamp"] // 1024) == (6 if name == "ev" else 5)
    b = run_batch(pkg, synth, g)
    variant, prepass = synth.info(pkg.INFO_LAST_VARIANT), synth.info(pkg.INFO_PREPASS)
    bad = dlc.check_batch(pkg, b, g["iq"], g["rep"], (1, 2, 4, 7))
    b.close()
    assert variant == dlc.dc.EV and prepass == 3
    assert not bad, "\n".join(bad)


def test_a_block_shorter_than_a_wavefront(pkg, synth, oracle, default_options):
    """nsamp = 40: lags of +-64 give zeros, lags of +-39 single terms"""
    g = case(pkg, oracle, "tiny")
    b = run_batch(pkg, synth, g)
    lags = (-64, -39, -1, 0, 1, 39, 64, 40)
    got = b.despread_lags(lags)
    b.close()
    want = pkg.despread_lags_host(g["iq"], g["rep"], 1, lags)
    assert (got == want).all()
    assert not got[..., 0, :].any() and not got[..., 6, :].any() and not got[..., 7, :].any()
    u, r = g["iq"].astype(np.int64), g["rep"].astype(np.int64)
    assert (got[:, :, 0, 5, 0] == u[:, None, 39, 0] * r[:, :, 0, 0] + u[:, None, 39, 1] * r[:, :, 0, 1]).all() and got[:, :, 0, 5].any()
    assert (got[:, :, 0, 1, 0] == u[:, None, 0, 0] * r[:, :, 39, 0] + u[:, None, 0, 1] * r[:, :, 39, 1]).all() and got[:, :, 0, 1].any()


@pytest.mark.parametrize("name", ["pd", "ev"])
def test_views_noise_and_interference(pkg, synth, oracle, default_options, name):
    """SC8 at shifts 0 and 5 and SC1, plain, with the noise fused and with noise and a CW emitter; sample0 far up and odd.  The
    sample at n + L carries the noise of position n + L: view_host applies it per position, before the shift."""
    g = case(pkg, oracle, name)
    nz = pkg.Noise(0xBEEF, (1 << 33) + 4321, pkg.noise_sigma(45.0, 1.0, g["delt"]), 1, 0)
    assert nz.sample0 > 1 << 33 and nz.sample0 & 1
    cw = pkg.InterfSet([pkg.interf_make(pkg.INTERF_CW, 6.0, 1.0e5, delt=g["delt"])], nz.shift, nz.sample0)
    views = [(v, n, j) for v in (pkg.OUT_SC16, pkg.OUT_SC8(0), pkg.OUT_SC8(5), pkg.OUT_SC1) for n, j in ((None, None), (nz, None), (nz, cw))]
    b = run_batch(pkg, synth, g)
    bad = dlc.check_batch(pkg, b, g["iq"], g["rep"], (2,), views=views)
    # the noise really differs from lag to lag: the column of lag L is not the noiseless one, and lag 0 is the impaired prompt sum
    noisy = b.despread_lags(LAGS, seg_tiles=2, noise=nz, interf=cw)
    prompt = b.despread(seg_tiles=2, noise=nz, interf=cw)
    clean = b.despread_lags(LAGS, seg_tiles=2)
    b.close()
    assert not bad, "\n".join(bad)
    assert (noisy[:, :, :, 3] == prompt).all()
    assert (noisy != clean).any(axis=(0, 1, 2, 4)).all()


def test_lag_0_is_the_prompt_call_and_nothing_is_written(pkg, synth, oracle, default_options):
    g = case(pkg, oracle, "pd")
    b = run_batch(pkg, synth, g)
    res = [(b.despread_lags((7, 0, 0, -7), seg_tiles=st), b.despread(seg_tiles=st), b.despread_lags([0], seg_tiles=st, view=pkg.OUT_SC1),
            b.despread(seg_tiles=st, view=pkg.OUT_SC1)) for st in (1, 3)]
    iq, _ = b.read()
    b.close()
    for got, want, got1, want1 in res:
        assert (got[:, :, :, 1] == want).all() and (got[:, :, :, 2] == want).all() and want.any()
        assert (got1[:, :, :, 0] == want1).all()
    assert (iq == g["iq"]).all()


def test_chunks_of_four_tiles_on_a_large_batch(pkg, synth, default_options):
    """What a wavefront does from its second tile on: reusing its LDS strip, adding several tiles of a segment into one running
    sum, flushing where a segment ends inside a chunk, taking another chunk.  The launcher keeps chunks of four tiles only
    while blocks * ceil(tiles / 4) >= 32 * compute units, and starts at most 16 * compute units workgroups of four wavefronts.
    4096 blocks of 33 tiles (the last 37 samples long, an odd count under one state per two tiles) are 36864 chunks: one
    workgroup per block, nine chunks for its four wavefronts.  Segments of 7 and 9 tiles end inside chunks.

    That is 138 M samples, too many for the CPU oracle, so the reference is the prompt call, which the parent's tests hold to
    the oracle, d_iq included: the column of lag L == gpsbb_batch_despread of the render moved L samples earlier within each
    block, zeros moved in (no noise here: noise goes by position), in SC16 and SC8.  Also: a repeated lag gives the same column
    twice, and with noise, and in SC1, the lag-0 column == the prompt call."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblocks, nsamp, fs = 4096, 32 * 1024 + 37, 25e6
    assert nblocks * -(-33 // 4) >= 32 * cus and 16 * cus <= nblocks   # chunks of four; one workgroup per block
    lags = (-64, -3, 0, 1, 64, 5, 1, 0)
    combos = ((pkg.OUT_SC16, 7), (pkg.OUT_SC16, 9), (pkg.OUT_SC8(5), 7))   # (not SC1: its view of a zero moved in is -1, not nothing)
    ch = pkg.synth_descriptors(nblocks, nch=16, seed=24)
    iq = torch.empty((nblocks, nsamp, 2), dtype=torch.int16, device="cuda")
    moved = torch.empty_like(iq)
    torch.cuda.synchronize()
    b = synth.batch(ch, 1.0 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    try:
        b.run(iq.data_ptr())
        synth.sync()
        assert synth.info(pkg.INFO_LAST_VARIANT) == dlc.dc.EV and synth.info(pkg.INFO_PREPASS) == 3
        got = {c: b.despread_lags(lags, seg_tiles=c[1], view=c[0], d_iq=iq.data_ptr()) for c in combos}
        for c in combos:
            assert got[c].shape == (nblocks, 16, -(-33 // c[1]), 8, 2)
            assert (got[c][:, :, :, 3] == got[c][:, :, :, 6]).all() and (got[c][:, :, :, 2] == got[c][:, :, :, 7]).all(), c
        for l, lag in enumerate(lags[:6]):
            moved.zero_()
            if lag >= 0:
                moved[:, :nsamp - lag] = iq[:, lag:]
            else:
                moved[:, -lag:] = iq[:, :nsamp + lag]
            torch.cuda.synchronize()
            for c in combos:
                want = b.despread(view=c[0], seg_tiles=c[1], d_iq=moved.data_ptr())
                assert want.any() and (got[c][:, :, :, l] == want).all(), (lag, c)
        nz = pkg.Noise(0xBEEF, (1 << 33) + 4321, pkg.noise_sigma(45.0, 1.0, 1.0 / fs), 1, 0)
        noisy = b.despread_lags(lags, seg_tiles=7, view=pkg.OUT_SC8(5), noise=nz, d_iq=iq.data_ptr())
        assert (noisy[:, :, :, 2] == b.despread(view=pkg.OUT_SC8(5), seg_tiles=7, noise=nz, d_iq=iq.data_ptr())).all()
        assert (noisy[:, :, :, 3] == noisy[:, :, :, 6]).all() and (noisy[:, :, :, 2] == noisy[:, :, :, 7]).all()
        sc1 = b.despread_lags(lags, seg_tiles=9, view=pkg.OUT_SC1, d_iq=iq.data_ptr())
        assert (sc1[:, :, :, 2] == b.despread(view=pkg.OUT_SC1, seg_tiles=9, d_iq=iq.data_ptr())).all()
        assert (sc1[:, :, :, 3] == sc1[:, :, :, 6]).all() and (sc1[:, :, :, 2] == sc1[:, :, :, 7]).all()
    finally:
        b.close()


@pytest.mark.parametrize("where,state_log2", [pytest.param("0", None, id="0"), pytest.param("1", None, id="1"),
                                              pytest.param("0", "2", id="0-g2")])
def test_the_exact_path_forced_often(pkg, where, state_log2):
    """The experiments build with the danger threshold raised from 40 to 2^22 units of 2^-32 (tests/test_despread_gpu.py's way, in
    a child process): about one channel-sample in five hundred takes ds_exact_sample's replica before the lags' sums are formed;
    the same numpy result at every lag, and the count says the path ran.  0-g2: the knob at 2, one state per four tiles for code
    and carrier alike — the equal-granule exact path at a place in the granule that is not its first tile."""
    env = dict(os.environ, GPSBB_PY_LIB="exp", GPSBB_DS_DANGER=str(1 << 22))
    if state_log2 is not None:
        env["GPSBB_EV_STATE_LOG2"] = state_log2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "despread_lags_check.py"), "--where", where], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bit-exact" in r.stdout
    if state_log2 is not None:   # the knob took: the breakpoint kernel's batches have one state per 2^state_log2 tiles, both kinds
        for name in ("ev", "ev_odd"):
            assert "%s: state granule log2 %s, the carrier's %s" % (name, state_log2, state_log2) in r.stdout, r.stdout[-2000:]
    n = [int(l.split(":")[1]) for l in r.stdout.splitlines() if l.startswith("exact-path samples")][0]
    assert n > 100, r.stdout[-2000:]


def test_refusals_leave_the_batch_usable(pkg, synth, oracle, default_options):
    L = pkg.lib()
    g = case(pkg, oracle, "pd")
    good = run_batch(pkg, synth, g)
    try:   # (a batch must not outlive its handle: a failure below would leave it to the collector)
        want = pkg.despread_lags_host(g["iq"], g["rep"], 2, LAGS)
        out = np.zeros(want.shape, np.int64)

        def rc_of(batch, lags, nlags=None, dst=out, view=0, seg_tiles=2):
            lg = np.ascontiguousarray([0] if lags is None else lags, np.int32)
            return L.gpsbb_batch_despread_lags(batch._b, None, view, None, None, seg_tiles, lg.ctypes.data if lags is not None else None,
                                               lg.size if nlags is None else nlags, None if dst is None else dst.ctypes.data)

        def ok():
            assert (good.despread_lags(LAGS, seg_tiles=2) == want).all()

        ok()
        for what, kw in (("nlags 0", dict(lags=[0], nlags=0)), ("nlags 9", dict(lags=[0] * 9)), ("nlags -1", dict(lags=[0], nlags=-1)),
                         ("a lag of 65", dict(lags=[0, 65])), ("a lag of -65", dict(lags=[-65])), ("lags NULL", dict(lags=None, nlags=1)),
                         ("out NULL", dict(lags=[0], dst=None)), ("seg_tiles 0", dict(lags=[0], seg_tiles=0)),
                         ("unknown format", dict(lags=[0], view=3 << 8))):
            assert rc_of(good, **kw) == BADARG, what
            ok()
        assert rc_of(good, [64, -64]) == 0
        assert L.gpsbb_batch_despread_lags(None, None, 0, None, None, 1, np.zeros(1, np.int32).ctypes.data, 1, out.ctypes.data) == BADARG
        fresh = synth.batch(g["ch"], g["delt"], g["nsamp"], flags=pkg.CHAIN_CARRIER)
        assert rc_of(fresh, [0]) == STATE
        fresh.close()
        fx = synth.batch(cc.fixed_of(g["ch"][0])[None, :], g["delt"], g["nsamp"], flags=pkg.FIXED_CARRIER)
        fx.run()
        synth.sync()
        assert rc_of(fx, [0]) == BADARG
        fx.close()
        ok()
        synth.set_option(pkg.OPT_SYNTH_KERNEL, 1)
        forced = run_batch(pkg, synth, g)
        assert synth.info(pkg.INFO_LAST_VARIANT) == cc.SYNTH and rc_of(forced, [0]) == BADARG
        forced.close()
        synth.set_option(pkg.OPT_SYNTH_KERNEL, 0)
        ok()
    finally:
        good.close()


def test_front_end_with_echoes_end_to_end(pkg, synth, oracle, default_options):
    """FrontEnd with two echoes (5 samples late on the satellite of slot 0, 2 samples late on that of slot 1) -> 3 chained blocks
    of 3 * 1024 + 37 samples with default options: the GPU's render == the oracle's, and in the GPU's own sums — the lag
    profile of the direct channels in the batch with the echoes less that in a batch without them, an exact subtraction — each
    echo's peak sits at its lag."""
    fs, nsamp = 2.6e6, 3 * 1024 + 37
    pkg.build_frontend()
    fe = pkg.FrontEnd(dlc.NAV, llh=dlc.SITE, max_chan=12)
    prns = [int(p) for p in fe.generate(1)["prn"][0, :2]]
    fe.close()
    fe = pkg.FrontEnd(dlc.NAV, llh=dlc.SITE, max_chan=12)
    fe.set_echoes([(prns[0], 5 * dlc.C_LIGHT / fs, 6.0, 0.3), (prns[1], 2 * dlc.C_LIGHT / fs, 3.0, 0.6, 0.5)])
    assert fe.block_chans == 14
    ch = fe.generate(3)
    fe.close()
    assert (ch["prn"][:, 12] == prns[0]).all() and (ch["prn"][:, 13] == prns[1]).all()
    want = oracle.fill_blocks(ch, 1.0 / fs, nsamp, chain=True)[0]
    lags = (-2, 0, 1, 2, 3, 4, 5, 7)
    b = synth.batch(ch, 1.0 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    iq, _ = b.read()
    with_echoes = b.despread_lags(lags, seg_tiles=4)
    b.close()
    assert (iq == want).all()
    bare = ch.copy()
    bare["prn"][:, 12:] = 0
    b = synth.batch(bare, 1.0 / fs, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    without = b.despread_lags(lags, seg_tiles=4)
    b.close()
    echo = (with_echoes - without)[:, :2, 0].astype(np.float64)   # [block, direct channel, lag, i/q]
    mag = np.hypot(echo[..., 0], echo[..., 1])
    assert (np.argmax(mag, axis=-1) == np.array([lags.index(5), lags.index(2)])[None, :]).all(), mag
