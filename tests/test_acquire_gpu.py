"""gpsbb_device_acquire on the GPU (k_acq): every comparison is == on integers against acquire_host fed with view_host's output
(tools/acq_check.py), on the smallest shapes at which the kernel can go wrong — a ragged delay tile, a ragged K-step, several
staged chunks and intervals, a mask — in every view, plain and impaired; the accumulators at their largest; ties; every refusal;
and end to end: six rendered satellites found by a search that is told nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1


def clips(pkg, synth):
    return synth.info(pkg.INFO_SC8_CLIPPED), synth.info(pkg.INFO_NOISE_CLIPPED)


def test_1_lane_map(pkg, synth):
    """Random int16 IQ (not a render) with +-32767 and -32768 in it, all 32 PRNs, N = 96, P = 40 (a whole delay tile and a ragged
    one), steps {0, +0x01234567, -0x0089abcd}, one interval: the whole grid and the rows == the mirror.  The data is asymmetric
    in every index, so a swapped row and column, a permuted k order or a wrong digit weight fails here."""
    iq, cfg = ac.lane_map_case(pkg)
    assert {32767, -32767, -32768} <= set(iq[:, 0].tolist()) and {32767, -32768} <= set(iq[:, 1].tolist())
    assert (cfg.prn_mask, cfg.ncoh, cfg.nlags, cfg.nnc, cfg.nbins) == (0xFFFFFFFF, 96, 40, 1, 3)
    rows, grid = ac.on_device(pkg, synth, iq, cfg)
    want_rows, want_grid = pkg.acquire_host(pkg.view_host(iq), cfg)
    bad = ac.compare(rows, grid, want_rows, want_grid)
    assert not bad, "\n".join(bad)
    assert len({int(x) for x in grid.reshape(-1)}) > 3800   # (32 * 3 * 40 cells, all different but for chance)
    # without the grid the rows are the same
    import torch
    t = torch.from_numpy(iq).cuda()
    assert synth.device_acquire(t.data_ptr(), iq.shape[0], cfg).tobytes() == want_rows.tobytes()


def test_2_ragged_k_and_intervals(pkg, synth):
    """N = 1000 (four staged chunks, the last K-step ragged), P = 70 (three delay tiles), 3 intervals, PRNs {1, 17, 32}, 2 bins,
    nsamp exactly nnc * N + P - 1; then the same with 5 spare samples of 0x7fff behind them, which no sum may see."""
    iq, cfg, n = ac.ragged_case(pkg)
    assert iq.shape[0] == n == cfg.nnc * cfg.ncoh + cfg.nlags - 1
    want_rows, want_grid = pkg.acquire_host(pkg.view_host(iq), cfg)
    rows, grid = ac.on_device(pkg, synth, iq, cfg)
    bad = ac.compare(rows, grid, want_rows, want_grid, "exact length")
    iq5, _, _ = ac.ragged_case(pkg, spare=5)
    assert iq5.shape[0] == n + 5 and (iq5[n:] == 0x7FFF).all() and (iq5[:n] == iq).all()
    rows5, grid5 = ac.on_device(pkg, synth, iq5, cfg)                  # the call is told of the spare samples
    bad += ac.compare(rows5, grid5, want_rows, want_grid, "5 spare samples, nsamp + 5")
    rows5, grid5 = ac.on_device(pkg, synth, iq5, cfg, nsamp=n)         # ... and not told
    bad += ac.compare(rows5, grid5, want_rows, want_grid, "5 spare samples, nsamp")
    assert not bad, "\n".join(bad)
    keep = [0, 16, 31]
    drop = [p for p in range(32) if p not in keep]
    assert not grid[drop].any() and rows[drop].tobytes() == bytes(32 * 2 * len(drop))
    assert grid[keep].all()


@pytest.mark.parametrize("impair", ["plain", "noise", "noise+chirp", "chirp"])
@pytest.mark.parametrize("name", ["sc16", "sc8", "sc1"])
def test_3_views(pkg, synth, name, impair):
    """The ragged shape in SC16, SC8(5) and SC1: plain, with a gpsbb_noise_t whose sample0 lies above 2^32, with noise and a chirp,
    and with the chirp alone.  Each == acquire_host(view_host(...)); the handle's clip counters do not move."""
    view = {"sc16": pkg.OUT_SC16, "sc8": pkg.OUT_SC8(5), "sc1": pkg.OUT_SC1}[name]
    iq, cfg, n = ac.ragged_case(pkg, view)
    delt = 1.0 / ac.FS
    nz = pkg._as_noise(ac.NOISE) if "noise" in impair else None
    assert ac.NOISE["sample0"] > 1 << 32
    js = None
    if "chirp" in impair:
        js = pkg.InterfSet([pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -0.2 * ac.FS, 0.27 * ac.FS, 301 * delt, delt=delt)], ac.NOISE["shift"],
                           ac.NOISE["sample0"])
    before = clips(pkg, synth)
    bad = ac.check(pkg, synth, iq, cfg, view, nz, js, what="%s %s" % (name, impair))
    assert not bad, "\n".join(bad)
    assert clips(pkg, synth) == before
    if impair != "plain":   # the impairment is really in the view
        assert (pkg.view_host(iq, view, nz, interf=js) != pkg.view_host(iq, view)).any()


def test_4_accumulator_range(pkg, synth):
    """Every component -32768, step 0, N = 65536, P = 32, one bin, all PRNs, shift = acq_min_shift: every digit plane's int32
    accumulator runs to 65536 terms of one sign pattern.  The grid == the closed form: y is one number for every sample, so
    S(p, L) = (the sum of PRN p's chips) * y for every L."""
    N, P = 65536, 32
    cfg = ac.make_cfg(pkg, (0,), N, P, 1, pkg.OUT_SC16)
    assert cfg.shift == pkg.acq_min_shift(pkg.OUT_SC16, N, 1)
    iq = np.full((N + P - 1, 2), -32768, np.int16)
    rows, grid = ac.on_device(pkg, synth, iq, cfg)
    sin512, cos512 = pkg.sincos_tables()
    c, s = int(cos512[0]), int(sin512[0])
    yi, yq = -32768 * c + -32768 * s, -32768 * c - -32768 * s
    xs = pkg.acq_chips(cfg, list(range(1, 33))).sum(axis=1)
    want = np.array([((int(x) * yi) >> cfg.shift) ** 2 + ((int(x) * yq) >> cfg.shift) ** 2 for x in xs], np.uint64)
    assert abs(yi) >= 1 << 22 and len(set(xs.tolist())) > 8
    assert (grid[:, 0, :] == want[:, None]).all()
    assert (rows["peak"][:, 0] == want).all() and not rows["lag"].any()
    tot = [int(w) * P for w in want]
    assert rows["sum_lo"][:, 0].tolist() == [t & ((1 << 64) - 1) for t in tot] and rows["sum_hi"][:, 0].tolist() == [t >> 64 for t in tot]


def test_5_ties(pkg, synth):
    """Zeros but for one sample at n0 = 100, N = 96, P = 40: S(p, L) = +-y[n0] for the delays with 0 <= n0 - L < N, that is L in
    5..39 — one value of M across two delay tiles — and 0 below: the smallest of the equal peaks' delays, 5, is reported.  A buffer
    of zeros gives zero rows with delay 0."""
    cfg = ac.make_cfg(pkg, (0x00abcdef,), 96, 40, 1, pkg.OUT_SC16)
    assert cfg.shift == 1   # (both components of the one sample are even, so y is, and (-y) >> 1 == -(y >> 1): the sign of the chip drops out)
    iq = np.zeros((96 + 40 - 1, 2), np.int16)
    rows, grid = ac.on_device(pkg, synth, iq, cfg)
    assert not grid.any() and rows.tobytes() == bytes(32 * 32)
    iq[100] = (1234, -566)
    rows, grid = ac.on_device(pkg, synth, iq, cfg)
    want_rows, want_grid = pkg.acquire_host(pkg.view_host(iq), cfg)
    bad = ac.compare(rows, grid, want_rows, want_grid)
    assert not bad, "\n".join(bad)
    assert not grid[:, 0, :5].any() and (grid[:, 0, 5:] == grid[0, 0, 5]).all() and grid[0, 0, 5] > 0
    assert (rows["lag"] == 5).all() and (rows["peak"] == grid[0, 0, 5]).all()


def test_6_refusals(pkg, synth, oracle):
    """Every GPSBB_E_BADARG of the definition; after each the handle still renders a block bit-exactly.  The buffer is large
    enough for every configuration tried, so a refusal that failed to refuse would still read inside it."""
    import torch
    L = pkg.lib()
    n = (1 << 20) + 1 + 64
    t = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    good = ac.make_cfg(pkg, ac.STEPS3, 96, 40, 1, pkg.OUT_SC16)
    rows = np.zeros((32, 64), pkg.ACQ_ROW_DTYPE)
    ch = pkg.synth_descriptors(1, nch=4, seed=31)[0]
    delt = 1.0 / ac.FS
    want_iq = oracle.fill_blocks(ch[None, :], delt, 1500)[0][0]

    def rc(cfg=good, ptr=t.data_ptr(), nsamp=n, view=0, nz=None, js=None, out=rows, null_cfg=False):
        return L.gpsbb_device_acquire(synth._h, C.c_void_p(ptr) if ptr else None, nsamp, view, None if nz is None else C.byref(nz),
                                      None if js is None else C.byref(js), None if null_cfg else C.byref(cfg),
                                      None if out is None else out.ctypes.data, None)

    def still_renders():
        iq, _ = synth.fill_block(ch, delt, 1500)
        assert (iq == want_iq).all()

    assert rc() == 0
    still_renders()
    nz_ok = pkg.Noise(1, 5, 100.0, 1, 0)
    cw = pkg.interf_make(pkg.INTERF_CW, 0.0, 1000.0, delt=delt)
    low = ac.make_cfg(pkg, (0,), 2600, 40, 2, pkg.OUT_SC16)
    assert low.shift == 6
    cases = [("d_iq NULL", dict(ptr=0)), ("cfg NULL", dict(null_cfg=True)), ("rows NULL", dict(out=None)),
             ("d_iq misaligned", dict(ptr=t.data_ptr() + 2)), ("nsamp one short", dict(nsamp=96 + 40 - 2)), ("nsamp 0", dict(nsamp=0)),
             ("nsamp < 0", dict(nsamp=-1)),
             ("prn_mask 0", dict(cfg=good.copy(prn_mask=0))), ("nbins 0", dict(cfg=good.copy(nbins=0))), ("nbins 65", dict(cfg=good.copy(nbins=65))),
             ("nbins < 0", dict(cfg=good.copy(nbins=-1))), ("code_step 0", dict(cfg=good.copy(code_step=0))),
             ("code_step above 1.5 chips", dict(cfg=good.copy(code_step=(3 << 31) + 1))), ("ncoh 0", dict(cfg=good.copy(ncoh=0))),
             ("ncoh 2^20 + 1", dict(cfg=good.copy(ncoh=(1 << 20) + 1, shift=31))), ("nlags 0", dict(cfg=good.copy(nlags=0))),
             ("nlags 32769", dict(cfg=good.copy(nlags=32769))), ("nnc 0", dict(cfg=good.copy(nnc=0))), ("nnc 65", dict(cfg=good.copy(nnc=65, shift=31))),
             ("shift -1", dict(cfg=good.copy(shift=-1))), ("shift 32", dict(cfg=good.copy(shift=32))),
             ("a shift below acq_min_shift", dict(cfg=low.copy(shift=5))),
             ("unknown format", dict(view=3 << 8)), ("a shift on SC16", dict(view=0x1000)), ("bits below the format", dict(view=1)),
             ("bits above the shift", dict(view=1 << 16)),
             ("noise sigma 0", dict(nz=pkg.Noise(1, 0, 0.0, 0, 0))), ("noise shift 8", dict(nz=pkg.Noise(1, 0, 100.0, 8, 0))),
             ("a set of 5 emitters", dict(js=_set_n(pkg, cw, 5))), ("a set's shift 8", dict(js=pkg.InterfSet([cw], 8, 0))),
             ("noise and set apart in sample0", dict(nz=nz_ok, js=pkg.InterfSet([cw], 1, 6))),
             ("noise and set apart in shift", dict(nz=nz_ok, js=pkg.InterfSet([cw], 2, 5)))]
    for what, kw in cases:
        assert rc(**kw) == BADARG, what
        still_renders()
    assert L.gpsbb_device_acquire(None, C.c_void_p(t.data_ptr()), n, 0, None, None, C.byref(good), rows.ctypes.data, None) == BADARG
    # the neighbours of the refusals are served
    assert rc(cfg=low) == 0 and rc(nsamp=96 + 40 - 1) == 0 and rc(nz=nz_ok, js=pkg.InterfSet([cw], 1, 5)) == 0
    assert rc(cfg=good.copy(code_step=3 << 31)) == 0 and rc(cfg=good.copy(shift=31)) == 0 and rc(view=pkg.OUT_SC8(15)) == 0
    still_renders()


def _set_n(pkg, e, n):
    js = pkg.InterfSet([e], 0, 0)
    js.n = n
    return js


@pytest.mark.parametrize("name", ["sc16", "sc1"])
def test_7_end_to_end(pkg, synth, name):
    """synth_descriptors(1, nch=6, seed=0xACC) rendered by the library at 2.6 MS/s, one block of 7800 samples, searched with
    acq_make(delt, -5000, 500, 21, 1e-3, 0, 2, view): N = P = 2600, two intervals, 21 bins, all 32 PRNs.  Per present PRN 1-6,
    acq_best gives the bin nearest f_carr and a delay within one sample, circularly in P, of ((1023 - code_phase) / (f_code *
    delt)) mod P; every present ratio is above twice the largest absent one.  What the mirror gives on the same render
    (tests/test_acquire.py): SC16 present min 85.1, absent max 15.0; SC1 57.8 and 11.3.  The rows of PRNs 1 and 32 == the
    mirror's (its prn_mask cut to those two: the whole mirror is too slow for this suite)."""
    view = {"sc16": pkg.OUT_SC16, "sc1": pkg.OUT_SC1}[name]
    ch = ac.e2e_descriptors(pkg)
    cfg = ac.e2e_cfg(pkg, view)
    assert (cfg.ncoh, cfg.nlags, cfg.nnc, cfg.nbins, cfg.prn_mask) == (2600, 2600, 2, 21, 0xFFFFFFFF)
    b = synth.batch(ch, 1.0 / ac.FS, ac.E2E_NSAMP)
    try:
        b.run()
        synth.sync()
        rows = synth.device_acquire(b.device_iq(), ac.E2E_NSAMP, cfg, view)
        iq, _ = b.read()
    finally:
        b.close()
    bad, present, absent = ac.e2e_findings(pkg, rows, cfg, ch)
    print("%s: present min %.1f, absent max %.1f" % (name, min(present.values()), max(absent.values())))
    assert not bad, "\n".join(bad)
    two = cfg.copy(prn_mask=ac.mask_of((1, 32)))
    want_rows, _ = pkg.acquire_host(pkg.view_host(iq[0], view), two)
    assert rows[[0, 31]].tobytes() == want_rows[[0, 31]].tobytes()
