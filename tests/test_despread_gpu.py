"""gpsbb_batch_despread on the GPU: every comparison is == on int64 against despread_host fed with the CPU oracle's replicas
(tools/despread_check.py) — the four model kernels' geometries on every pre-pass, the whole corner table of the contract, the
views with noise fused and on an external buffer, grazing states, the exact path made common, what the call must leave alone
and what it refuses."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import contract_corners as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_check as dc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG, STATE = -1, -7
PREPASS_OF = {0: 3, 1: 1, 2: 2, 3: 3}   # GPSBB_OPT_SEED_WHERE -> GPSBB_INFO_PREPASS (include/gpsbb.h: the lap-parallel pre-pass at every size
                                        # wherever a model kernel renders)


@pytest.fixture
def default_options(pkg, synth):
    yield
    synth.set_option(pkg.OPT_SEED_WHERE, 0)
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 0)


_cases = {}


def geometry(pkg, oracle, name):
    """one of tools/despread_check.py's geometries with the oracle's chained render and replicas, once per session"""
    if name not in _cases:
        g = [g for g in dc.geometries(pkg) if g["name"] == name][0]
        delt = 1.0 / g["fs"]
        iq, _, hz = oracle.fill_blocks(g["ch"], delt, g["nsamp"], chain=True)
        assert hz["itable_512"] == 0 and hz["dwrd_oob"] == 0
        _cases[name] = dict(g, delt=delt, iq=iq, rep=dc.replicas(oracle, g["ch"], delt, g["nsamp"], chain=True))
    return _cases[name]


def run_batch(pkg, synth, g, flags=None):
    b = synth.batch(g["ch"], g["delt"], g["nsamp"], flags=pkg.CHAIN_CARRIER if flags is None else flags)
    b.run()
    synth.sync()
    return b


@pytest.mark.parametrize("where", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["pd wide", "pd narrow", "ev", "ev dense"])
def test_geometries_on_every_prepass(pkg, synth, oracle, default_options, name, where):
    """2.6 MS/s x 300 000 x 12 ch, 3 MS/s x 16 ch, 25 MS/s x 16 ch (a state per two tiles behind the lap pre-pass) and a block
    with dense channels, chained over 3 - 4 blocks with an idle channel, a pause and a PRN hand-over; nsamp a multiple neither
    of 1024 nor of the segment; seg_tiles 1, 3 and the whole block; the kernel and the pre-pass that were meant."""
    g = geometry(pkg, oracle, name)
    synth.set_option(pkg.OPT_SEED_WHERE, where)
    b = run_batch(pkg, synth, g)
    assert synth.info(pkg.INFO_LAST_VARIANT) == g["variant"]
    assert synth.info(pkg.INFO_PREPASS) == PREPASS_OF[where]
    ntiles = math.ceil(g["nsamp"] / 1024)
    assert g["nsamp"] % 1024 and g["nsamp"] % 3072
    bad = dc.check_batch(pkg, synth, b, g["iq"], g["rep"], (1, 3, ntiles))
    got = b.despread(seg_tiles=ntiles + 5)   # longer than the block: one segment all the same
    assert got.shape == (g["ch"].shape[0], g["ch"].shape[1], 1, 2) and (got == pkg.despread_host(g["iq"], g["rep"], ntiles)).all()
    assert not got[:, 3].any() and not got[1, 5].any()   # idle channels: zeros
    # the signal is in P.i: gain * sum |r|^2 to within the cross-correlation
    act = g["ch"]["prn"] > 0
    assert (got[..., 0, 0][act] > 0).all()
    # the run's own output again after the despread: nothing was touched
    iq, _ = b.read()
    b.close()
    assert not bad, "\n".join(bad)
    assert (iq == g["iq"]).all()


def test_every_corner_of_the_contract(pkg, synth, oracle, default_options):
    """tests/contract_corners.py's table, every case: float-carrier cases of a model kernel despread bit-exactly, k_synth's are
    refused, the accumulator's are refused; the three lists are non-empty and cover the table."""
    T = cc.table(pkg)
    exact, synth_refused, fixed_refused, bad = [], [], [], []
    for k, c in enumerate(T):
        delt, nsamp = 1.0 / c["fs"], c["nsamp"]
        flags = pkg.FIXED_CARRIER if c["fixed"] else 0
        b = synth.batch(c["ch"][None, :], delt, nsamp, flags=flags)
        b.run()
        synth.sync()
        v = synth.info(pkg.INFO_LAST_VARIANT)
        if v != c["variant"]:
            bad.append("%s: rendered by %s, the table says %s" % (c["name"], cc.VARIANT_NAMES.get(v, v), cc.VARIANT_NAMES[c["variant"]]))
        if c["fixed"] or c["variant"] == cc.SYNTH:
            with pytest.raises(pkg.GpsbbError) as e:
                b.despread()
            if e.value.rc != BADARG:
                bad.append("%s: refused with %d" % (c["name"], e.value.rc))
            (fixed_refused if c["fixed"] else synth_refused).append(k)
        else:
            assert c["variant"] in (cc.EV, cc.EV_DENSE, cc.PD_WIDE, cc.PD_NARROW)
            iq, _, _ = oracle.fill_blocks(c["ch"], delt, nsamp)
            rep = dc.replicas(oracle, c["ch"], delt, nsamp)
            bad += ["%s: %s" % (c["name"], f) for f in dc.check_batch(pkg, synth, b, iq, rep, (1, 5))]
            exact.append(k)
        b.close()
    assert exact and synth_refused and fixed_refused
    assert sorted(exact + synth_refused + fixed_refused) == list(range(len(T)))
    assert not bad, "%d findings:\n%s" % (len(bad), "\n".join(bad[:60]))


@pytest.mark.parametrize("name,shift", [("pd wide", 0), ("ev", 1)])
def test_views_with_noise_fused_and_on_an_external_buffer(pkg, synth, oracle, default_options, name, shift):
    """SC16, SC8 at shifts 0 / 5 / 15 and SC1; without noise, with the noise fused into the despreading, and on a buffer
    gpsbb_device_noise filled: the last two give the same sums, view_host's; the stream position far up and odd."""
    import torch
    g = geometry(pkg, oracle, name)
    nb = g["ch"].shape[0]
    nz = pkg.Noise(0xBEEF, (1 << 33) + 4321, pkg.noise_sigma(45.0, 1.0, g["delt"]), shift, 0)
    assert nz.sample0 > 1 << 33 and nz.sample0 & 1
    b = run_batch(pkg, synth, g)
    ext = torch.zeros(nb * g["nsamp"] * 2, dtype=torch.int16, device="cuda")
    synth.device_noise(b.device_iq(), nb, g["nsamp"], nz, d_dst=ext.data_ptr())
    noisy, _ = pkg.apply_noise(g["iq"], nz.seed, nz.sample0, nz.sigma, nz.shift)
    assert (ext.cpu().numpy().reshape(noisy.shape) == noisy).all()
    bad = []
    for view in (pkg.OUT_SC16, pkg.OUT_SC8(0), pkg.OUT_SC8(5), pkg.OUT_SC8(15), pkg.OUT_SC1):
        want = pkg.despread_host(pkg.view_host(g["iq"], view, nz), g["rep"], 3)
        fused = b.despread(view=view, noise=nz, seg_tiles=3)
        external = b.despread(view=view, seg_tiles=3, d_iq=ext.data_ptr())
        plain = b.despread(view=view, seg_tiles=3)
        if not (fused == want).all():
            bad.append("view 0x%x: noise fused differs from view_host" % view)
        if not (external == fused).all():
            bad.append("view 0x%x: the external noisy buffer gives other sums than the fused noise" % view)
        if not (plain == pkg.despread_host(pkg.view_host(g["iq"], view), g["rep"], 3)).all():
            bad.append("view 0x%x: without noise" % view)
    b.close()
    del ext
    assert not bad, "\n".join(bad)


GRAZE_OFFSETS = [0, 1, -1, 2, -2, 3, -3, 4, -4, 8, -8, 16, -16, 20, -20, 24, -24, 32, -32, 39, -39, 40, -40, 41, -41, 48, -48]


@pytest.mark.parametrize("fs,nch,nsamp,dopp,samples", [
    (25e6, 16, 70001, 12000.0, [16, 15, 1008, 1023, 1024, 1025, 2047, 2048, 70000, 69985, 5000, 777]),   # k_synth_ev, a state per two tiles
    (15.8565e6, 12, 60000, 5000.0, None),                                                                # k_synth_ev_dense
    (2.6e6, 12, 100000, 20000.0, None),                                                                  # k_synth_pd wide
    (2.6e6, 16, 100000, 300000.0, [64, 63, 960, 1023, 1024, 1087, 99999, 99936, 4097]),                  # ... narrow, fast carriers
])
def test_states_that_graze_an_integer_at_a_sample(pkg, synth, oracle, default_options, fs, nch, nsamp, dopp, samples):
    """The adversarial case: descriptors aimed so that the REFERENCE's carrier phase * 512 or code phase is within 0 .. +-48 units
    of 2^-32 of an integer exactly at a sample, either side of it, inside the danger band (40 units of the biased model's low
    word: the exact path) and just outside it (the model is trusted)."""
    ch, targets = pkg.grazing_descriptors(5, nch, fs, nsamp, GRAZE_OFFSETS, seed=int(fs) % 1000 + nch + 1, max_doppler=dopp, samples=samples)
    assert all(abs(t[5] - t[4]) <= 0.3 for t in targets), "the generator missed a target"
    delt = 1.0 / fs
    iq, _, _ = oracle.fill_blocks(ch, delt, nsamp)
    rep = dc.replicas(oracle, ch, delt, nsamp)
    for where in (0, 1):
        synth.set_option(pkg.OPT_SEED_WHERE, where)
        b = synth.batch(ch, delt, nsamp)
        b.run()
        synth.sync()
        bad = dc.check_batch(pkg, synth, b, iq, rep, (1, 4))
        b.close()
        assert not bad, "seed where %d:\n%s" % (where, "\n".join(bad))
    synth.hazards(reset=True)


@pytest.mark.parametrize("where,state_log2", [pytest.param("0", None, id="0"), pytest.param("1", None, id="1"),
                                              pytest.param("0", "2", id="0-g2")])
def test_the_exact_path_forced_often(pkg, where, state_log2):
    """The experiments build with the danger threshold raised from 40 to 2^22 units of 2^-32: about one sample in five hundred
    of every channel is recomputed by ds_exact_sample, in nearly every tile; same sums.  Once per table layout: a state per two
    tiles behind the lap pre-pass (0), a state per tile behind the row walks (1) — and with the knob at 2 (0-g2) a state per four
    tiles for code and carrier alike: the equal-granule exact path at a place in the granule that is not its first tile."""
    env = dict(os.environ, GPSBB_PY_LIB="exp", GPSBB_DS_DANGER=str(1 << 22))
    if state_log2 is not None:
        env["GPSBB_EV_STATE_LOG2"] = state_log2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "despread_check.py"), "--where", where, "--views"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bit-exact" in r.stdout
    if state_log2 is not None:   # the knob took: the breakpoint kernel's batches have one state per 2^state_log2 tiles, both kinds
        assert "ev: state granule log2 %s, the carrier's %s" % (state_log2, state_log2) in r.stdout, r.stdout[-2000:]
    n = [int(l.split(":")[1]) for l in r.stdout.splitlines() if l.startswith("exact-path samples")][0]
    # the last despread of each of the four batches looked at all its channel-samples: two tests of 2^22 / 2^32 each
    assert n > 10000, r.stdout[-2000:]


def test_it_only_reads(pkg, synth, oracle, default_options):
    """The buffer's digests, the clip counters, the exact-run counter, the hazards and a second gpsbb_batch_read are the same
    before and after despreading in every view, with noise."""
    g = geometry(pkg, oracle, "pd narrow")
    nb = g["ch"].shape[0]
    b = run_batch(pkg, synth, g)
    nz = pkg.Noise(3, 99, 20000.0, 0, 0)   # (sigma large enough to saturate, had the call counted it)

    def snapshot():
        iq, st = b.read()
        return (synth.device_digest(b.device_iq(), nb, g["nsamp"]).tolist(), synth.info(pkg.INFO_SC8_CLIPPED), synth.info(pkg.INFO_NOISE_CLIPPED),
                synth.info(pkg.INFO_EXACT_RUNS), synth.info(pkg.INFO_TILES_RENDERED), synth.hazards(), iq.tobytes(), st.tobytes(),
                synth.info(pkg.INFO_LAST_VARIANT), synth.info(pkg.INFO_PREPASS))

    before = snapshot()
    assert before[0] == pkg.block_digest_host(g["iq"]).tolist()
    for view in (pkg.OUT_SC16, pkg.OUT_SC8(0), pkg.OUT_SC1):
        b.despread(view=view, noise=nz, seg_tiles=2)
        b.despread(view=view)
    assert snapshot() == before
    b.close()


def test_refusals_leave_the_handle_usable(pkg, synth, oracle, default_options):
    """Every refusal of include/gpsbb.h, each followed by a successful call on the same handle (and, where there is one, on the
    same batch)."""
    L = pkg.lib()
    g = geometry(pkg, oracle, "pd narrow")
    nb, nch = g["ch"].shape
    want = pkg.despread_host(g["iq"], g["rep"], 2)
    out = np.zeros(want.shape, np.int64)
    good = run_batch(pkg, synth, g)

    def ok():
        assert (good.despread(seg_tiles=2) == want).all()

    def rc_of(batch, view=0, nz=None, seg_tiles=2, dst=out, d_iq=None):
        return L.gpsbb_batch_despread(batch._b, d_iq, view, None if nz is None else C.byref(nz), seg_tiles, None if dst is None else dst.ctypes.data)

    ok()
    fresh = synth.batch(g["ch"], g["delt"], g["nsamp"], flags=pkg.CHAIN_CARRIER)
    assert rc_of(fresh) == STATE                      # not run
    fresh.run()
    synth.sync()
    assert (fresh.despread(seg_tiles=2) == want).all()   # ... and the same batch once it has
    fresh.close()
    for what, kw in (("seg_tiles 0", dict(seg_tiles=0)), ("seg_tiles -3", dict(seg_tiles=-3)), ("unknown format", dict(view=3 << 8)),
                     ("a shift on SC1", dict(view=pkg.OUT_SC1 | (4 << 12))), ("a shift above 15", dict(view=(1 << 8) | (16 << 12))),
                     ("batch flags in the view", dict(view=pkg.CHAIN_CARRIER)), ("sigma 0", dict(nz=pkg.Noise(1, 0, 0.0, 0, 0))),
                     ("sigma NaN", dict(nz=pkg.Noise(1, 0, float("nan"), 0, 0))), ("noise shift 8", dict(nz=pkg.Noise(1, 0, 100.0, 8, 0))),
                     ("out NULL", dict(dst=None))):
        assert rc_of(good, **kw) == BADARG, what
        ok()
    assert L.gpsbb_batch_despread(None, None, 0, None, 1, out.ctypes.data) == BADARG
    # the accumulator's batches
    fx = synth.batch(cc.fixed_of(g["ch"][0])[None, :], g["delt"], g["nsamp"], flags=pkg.FIXED_CARRIER)
    fx.run()
    synth.sync()
    assert rc_of(fx) == BADARG
    fx.close()
    ok()
    # k_synth by the plan (1 MS/s: 1.023 chips per sample) and by the option
    slow = synth.batch(g["ch"], 1e-6, 20000, flags=pkg.CHAIN_CARRIER)
    slow.run()
    synth.sync()
    assert synth.info(pkg.INFO_LAST_VARIANT) == cc.SYNTH and rc_of(slow) == BADARG
    slow.close()
    ok()
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 1)
    forced = run_batch(pkg, synth, g)
    assert synth.info(pkg.INFO_LAST_VARIANT) == cc.SYNTH and rc_of(forced) == BADARG
    forced.close()
    synth.set_option(pkg.OPT_SYNTH_KERNEL, 0)
    ok()
    # a run into the caller's buffer has to be named
    import torch
    ext = torch.zeros(nb * g["nsamp"] * 2, dtype=torch.int16, device="cuda")
    good.run(ext.data_ptr())
    synth.sync()
    assert rc_of(good) == STATE
    assert (good.despread(seg_tiles=2, d_iq=ext.data_ptr()) == want).all()
    good.run()
    synth.sync()
    ok()
    good.close()
    del ext


def test_the_cn0_a_receiver_finds_on_the_gpu(pkg, synth):
    """tests/test_despread.py's statement once on the GPU's own sums: batch -> noise -> despread -> gpsbb_cn0_estimate, every
    channel within 0.46 dB of what was asked for (scaled by its gain, less the cross-correlation), SC1 < SC8 <= SC16 + 0.46."""
    import test_despread as td
    delt = 1.0 / td.FS
    ch = pkg.synth_descriptors(td.NBLOCKS, nch=td.NCH, seed=45)
    ch["gain"] = ch["gain"][0]
    sigma = pkg.noise_sigma(td.CN0, 1.0, delt)
    nz = pkg.Noise(45, 0, sigma, 0, 0)
    T = 1024 * td.SEG_TILES * delt
    b = synth.batch(ch, delt, td.NSAMP, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    clean = td.whole(b.despread(seg_tiles=td.SEG_TILES))
    est = {}
    for name, fmt in (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(6)), ("sc1", pkg.OUT_SC1)):
        p = td.whole(b.despread(view=fmt, noise=nz, seg_tiles=td.SEG_TILES))
        est[name] = np.array([pkg.cn0_estimate(p[i], T) for i in range(td.NCH)])
    b.close()
    want = np.array([td.expected_cn0(pkg, float(ch["gain"][0, i]), clean[i, :, 1], sigma) for i in range(td.NCH)])
    resid = est["sc16"] - want
    print("\nsc16 residuals %+.2f .. %+.2f dB; sc8 >> 6 %+.2f .. %+.2f; sc1 %+.2f .. %+.2f" % (
        resid.min(), resid.max(), (est["sc8"] - est["sc16"]).min(), (est["sc8"] - est["sc16"]).max(),
        (est["sc1"] - est["sc16"]).min(), (est["sc1"] - est["sc16"]).max()))
    assert np.isfinite(resid).all() and (np.abs(resid) <= td.TOL_DB).all(), resid
    assert (est["sc1"] < est["sc8"]).all() and (est["sc8"] <= est["sc16"] + td.TOL_DB).all()
