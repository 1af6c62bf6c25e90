"""The acquisition search without a GPU: the host helpers (gpsbb_acq_make, gpsbb_acq_min_shift, gpsbb_acq_best) against Python
integers, every refusal of theirs, and the numpy mirror acquire_host — against a third, brute-force restatement of the
definition in Python integers, and end to end on the CPU oracle's render of six satellites."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402

BADARG = -1
WMAX = {"sc16": 32768, "sc8": 128, "sc1": 1}


def views(pkg):
    return {"sc16": pkg.OUT_SC16, "sc8": pkg.OUT_SC8(5), "sc1": pkg.OUT_SC1}


def min_shift_int(wmax, ncoh, nnc):
    b = ncoh * wmax * 1024
    a = 0
    while 2 * nnc * ((b >> a) + 1) ** 2 >= 1 << 64:
        a += 1
    return a


def test_min_shift_against_python_integers(pkg):
    v = views(pkg)
    assert pkg.acq_min_shift(v["sc16"], 2600, 2) == 6 and pkg.acq_min_shift(v["sc1"], 2600, 2) == 0   # the header's examples
    for name, view in v.items():
        for ncoh in (1, 96, 2600, 3000, 25000, 65536, (1 << 20) - 1, 1 << 20):
            for nnc in (1, 2, 3, 64):
                assert pkg.acq_min_shift(view, ncoh, nnc) == min_shift_int(WMAX[name], ncoh, nnc), (name, ncoh, nnc)
    assert pkg.acq_min_shift(v["sc16"], 1 << 20, 64) == min_shift_int(32768, 1 << 20, 64) <= 31


@pytest.mark.parametrize("fs", [2.6e6, 3.0e6, 25e6])
def test_make_against_python_integers(pkg, fs):
    delt = 1.0 / fs
    for name, view in views(pkg).items():
        cfg = pkg.acq_make(delt, -5000.0, 500.0, 21, 1e-3, 0, 2, view)
        cstep = int(np.rint(math.ldexp(1.023e6 * delt, 32)))
        ncoh = int(np.rint(1e-3 / delt))
        assert (cfg.prn_mask, cfg.nbins, cfg.code_step, cfg.ncoh, cfg.nnc) == (0xFFFFFFFF, 21, cstep, ncoh, 2)
        assert cfg.nlags == -((-1023 << 32) // cstep) and cfg.nlags == round(fs / 1000)   # one code period, rounded up
        assert cfg.shift == min_shift_int(WMAX[name], ncoh, 2)
        for k in range(21):
            want = int(np.rint(math.ldexp((-5000.0 + k * 500.0) * delt, 32)))
            assert cfg.step[k] == want and (k != 10 or want == 0)
        assert not any(cfg.step[k] for k in range(21, 64))
    cfg = pkg.acq_make(delt, 1234.5, -7.25, 64, 2.5e-4, 333, 64, pkg.OUT_SC16)
    assert (cfg.nbins, cfg.nlags, cfg.nnc, cfg.ncoh) == (64, 333, 64, int(np.rint(2.5e-4 / delt)))
    assert cfg.step[63] == int(np.rint(math.ldexp((1234.5 - 63 * 7.25) * delt, 32)))
    edge = pkg.acq_make(delt, -0.4999 * fs, 0.9998 * fs, 2, 1e-3, 1, 1)    # both ends of the step's range, as two's complement
    assert edge.step[0] == int(np.rint(math.ldexp(-0.4999 * fs * delt, 32))) < 0 < edge.step[1]


def test_every_refusal_of_the_host_helpers(pkg):
    L = pkg.lib()
    v = views(pkg)
    for what, args in (("unknown format", (3 << 8, 100, 1)), ("a shift on SC16", (0x1000, 100, 1)), ("a shift on SC1", (pkg.OUT_SC1 | 0x1000, 100, 1)),
                       ("bits below the format", (1, 100, 1)), ("bits above the shift", (1 << 16, 100, 1)), ("ncoh 0", (0, 0, 1)),
                       ("ncoh 2^20 + 1", (0, (1 << 20) + 1, 1)), ("nnc 0", (0, 100, 0)), ("nnc 65", (0, 100, 65)), ("ncoh < 0", (0, -5, 1))):
        assert L.gpsbb_acq_min_shift(*args) == BADARG, what
    assert L.gpsbb_acq_min_shift(pkg.OUT_SC8(15), 1 << 20, 64) >= 0
    cfg = pkg.AcqCfg()
    cfg.nbins = 77   # (left as it was by every refusal)
    good = dict(delt=1 / 2.6e6, f_min=-5000.0, f_step=500.0, nbins=21, coh=1e-3, nlags=0, nnc=2, view=0)

    def make(ptr=C.byref(cfg), **kw):
        a = dict(good, **kw)
        return L.gpsbb_acq_make(ptr, a["delt"], a["f_min"], a["f_step"], a["nbins"], a["coh"], a["nlags"], a["nnc"], a["view"])

    for what, kw in (("delt 0", dict(delt=0.0)), ("delt < 0", dict(delt=-1e-6)), ("delt NaN", dict(delt=math.nan)), ("delt inf", dict(delt=math.inf)),
                     ("f_min NaN", dict(f_min=math.nan)), ("f_step inf", dict(f_step=math.inf)), ("|f delt| = 0.5", dict(delt=2.0 ** -21, f_min=-2.0 ** 20)), ("f beyond", dict(f_min=-1.4e6)),
                     ("a later bin beyond 0.5", dict(f_step=1.0e5)), ("nbins 0", dict(nbins=0)), ("nbins 65", dict(nbins=65)),
                     ("coh 0", dict(coh=0.0)), ("coh NaN", dict(coh=math.nan)), ("coh < 0", dict(coh=-1e-3)), ("ncoh rounds to 0", dict(coh=1e-8)),
                     ("ncoh above 2^20", dict(coh=0.5)), ("nlags 32769", dict(nlags=32769)), ("nnc 0", dict(nnc=0)), ("nnc 65", dict(nnc=65)),
                     ("unknown format", dict(view=3 << 8)), ("code step above 1.5 chips", dict(delt=2e-6)),
                     ("a code period above 32768 samples", dict(delt=1e-8, coh=1e-4, f_min=0.0, f_step=0.0))):
        assert make(**kw) == BADARG, what
        assert cfg.nbins == 77
    assert make(ptr=None) == BADARG
    assert make() == 0 and cfg.nbins == 21
    assert make(delt=1e-8, coh=1e-4, f_min=0.0, f_step=0.0, nlags=32768) == 0   # the same rate with the delays named
    rows = np.zeros((32, 21), pkg.ACQ_ROW_DTYPE)
    b = C.c_int()
    assert L.gpsbb_acq_best(None, C.byref(cfg), 1, C.byref(b), None, None, None) == BADARG
    assert L.gpsbb_acq_best(rows.ctypes.data, None, 1, C.byref(b), None, None, None) == BADARG
    for prn in (0, 33, -1):
        assert L.gpsbb_acq_best(rows.ctypes.data, C.byref(cfg), prn, C.byref(b), None, None, None) == BADARG
    for f, val in (("nbins", 0), ("nbins", 65), ("nlags", 0), ("nlags", 32769)):
        assert L.gpsbb_acq_best(rows.ctypes.data, C.byref(cfg.copy(**{f: val})), 1, C.byref(b), None, None, None) == BADARG, (f, val)
    assert L.gpsbb_acq_best(rows.ctypes.data, C.byref(cfg), 32, None, None, None, None) == 0   # every out pointer may be NULL
    assert v["sc16"] == 0


def test_best_on_hand_made_rows(pkg):
    cfg = ac.make_cfg(pkg, (0, 1, 2, 3), 100, 10, 1, pkg.OUT_SC16)
    rows = np.zeros((32, 4), pkg.ACQ_ROW_DTYPE)
    # PRN 3: the largest peak twice, in bins 1 and 3: the lowest bin wins, with that row's lag
    rows["peak"][2] = (5, 900, 7, 900)
    rows["lag"][2] = (1, 4, 2, 9)
    rows["sum_lo"][2] = (10, 1000, 20, 970)
    assert pkg.acq_best(rows, cfg, 3) == (1, 4, 900, 900 / (2000 / 40))
    # PRN 4: all zero: bin 0, lag 0, ratio 0 and no division by zero
    assert pkg.acq_best(rows, cfg, 4) == (0, 0, 0, 0.0)
    # PRN 32: a sum that needs sum_hi, and the carries of adding four rows
    rows["peak"][31] = (1 << 63, (1 << 64) - 1, 3, 4)
    rows["lag"][31] = (0, 9, 0, 0)
    rows["sum_lo"][31] = ((1 << 64) - 1, (1 << 64) - 1, 5, 0)
    rows["sum_hi"][31] = (2, 0, 0, 1)
    tot = (2 << 64) + (1 << 64) - 1 + (1 << 64) - 1 + 5 + (1 << 64)
    b, lag, peak, ratio = pkg.acq_best(rows, cfg, 32)
    assert (b, lag, peak) == (1, 9, (1 << 64) - 1)
    assert ratio == float((1 << 64) - 1) / (float(tot) / 40.0)
    # rows of other PRNs are not looked at
    assert pkg.acq_best(rows, cfg, 1) == (0, 0, 0, 0.0)


def brute_cell(pkg, u, cfg, prn, k, lag):
    """M(prn, k, lag) of the definition in Python integers, term by term"""
    sin512, cos512 = pkg.sincos_tables()
    ca = pkg.codegen(prn)
    N, a = int(cfg.ncoh), int(cfg.shift)
    step = int(cfg.step[k])
    m_tot = 0
    for i in range(int(cfg.nnc)):
        si = sq = 0
        for m in range(N):
            r = i * N + m
            x = 1 if ca[((int(cfg.code_step) * r) >> 32) % 1023] else -1
            n = r + lag
            idx = ((step * n) & 0xFFFFFFFF) >> 23
            c, s = int(cos512[idx]), int(sin512[idx])
            wi, wq = int(u[n, 0]), int(u[n, 1])
            si += x * (wi * c + wq * s)
            sq += x * (wq * c - wi * s)
        m_tot += (si >> a) ** 2 + (sq >> a) ** 2
    return m_tot


def test_mirror_against_brute_force_and_both_products(pkg):
    """acquire_host in int64 == acquire_host through float64 products (exact below 2^53) on the GPU tests' shapes, and both == the
    definition in Python integers on cells at the corners of the grid; rows follow from the grid."""
    for (iq, cfg), nsamp in ((ac.lane_map_case(pkg), None), (ac.ragged_case(pkg, spare=5)[:2], 3069)):
        u = pkg.view_host(iq[:nsamp])
        rows, grid = pkg.acquire_host(u, cfg, blas=True)
        rows_i, grid_i = pkg.acquire_host(u, cfg, blas=False)
        assert (grid == grid_i).all() and rows.tobytes() == rows_i.tobytes() and grid.any()
        P, nb = cfg.nlags, cfg.nbins
        prns = [p for p in range(1, 33) if (cfg.prn_mask >> (p - 1)) & 1]
        for prn, k, lag in ((prns[0], 0, 0), (prns[-1], nb - 1, P - 1), (prns[len(prns) // 2], 1, 33), (prns[0], nb - 1, 31), (prns[-1], 0, 32)):
            assert int(grid[prn - 1, k, lag]) == brute_cell(pkg, u, cfg, prn, k, lag), (prn, k, lag)
        for p in range(32):
            if p + 1 not in prns:
                assert not grid[p].any() and rows[p].tobytes() == bytes(32 * nb)
                continue
            for k in range(nb):
                g = [int(x) for x in grid[p, k]]
                tot = sum(g)
                assert (int(rows["peak"][p, k]), int(rows["lag"][p, k])) == (max(g), g.index(max(g)))
                assert (int(rows["sum_lo"][p, k]), int(rows["sum_hi"][p, k])) == (tot & ((1 << 64) - 1), tot >> 64)


def test_mirror_refuses_a_short_buffer(pkg):
    iq, cfg = ac.lane_map_case(pkg)
    with pytest.raises(ValueError):
        pkg.acquire_host(pkg.view_host(iq[:-1]), cfg)


@pytest.mark.parametrize("name", ["sc16", "sc1"])
def test_end_to_end_on_the_oracles_render(pkg, oracle, name):
    """synth_descriptors(1, nch=6, seed=0xACC) rendered by the CPU oracle at 2.6 MS/s, 7800 samples; acq_make(delt, -5000, 500, 21,
    1e-3, 0, 2, view): N = P = 2600, two intervals.  All six present PRNs are found at the bin nearest f_carr and within one
    sample of the descriptor's delay, and every present ratio is above twice the largest absent one.  The mirror's ratios
    (peak over the PRN's mean cell), as this test prints them:

        view   present min   absent max
        SC16   85.1          15.0
        SC1    57.8          11.3
    """
    view = views(pkg)[name]
    ch = ac.e2e_descriptors(pkg)
    iq = oracle.fill_blocks(ch, 1.0 / ac.FS, ac.E2E_NSAMP, chain=True)[0][0]
    cfg = ac.e2e_cfg(pkg, view)
    assert (cfg.ncoh, cfg.nlags, cfg.nnc, cfg.nbins) == (2600, 2600, 2, 21)
    rows, _ = pkg.acquire_host(pkg.view_host(iq, view), cfg)
    bad, present, absent = ac.e2e_findings(pkg, rows, cfg, ch)
    print("%s: present min %.1f, absent max %.1f" % (name, min(present.values()), max(absent.values())))
    assert not bad, "\n".join(bad)
