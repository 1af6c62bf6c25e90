"""Despreading on the CPU: the replica recipe against the oracle's render, despread_host against a per-sample loop, the host
calls of the ABI (gpsbb_despread_segments, gpsbb_cn0_estimate) against numpy, and the receiver's view end to end — the C/N0 a
channel really has in a noisy render, per output format."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_check as dc  # noqa: E402


class Corr(C.Structure):
    _fields_ = [("i", C.c_int64), ("q", C.c_int64)]


@pytest.mark.parametrize("fs,nch,nsamp,nblocks", [(2.6e6, 12, 300000, 9), (25e6, 16, 2500000, 10)])
def test_the_render_is_the_sum_of_the_scaled_replicas(pkg, oracle, fs, nch, nsamp, nblocks):
    """sum_i trunc(gain_i * r_i) == the oracle's render at every sample of a second of oracle time, chained, with r_i the
    oracle's render of channel i alone at gain 1.0: what the definition in include/gpsbb.h says a replica is."""
    ch = pkg.synth_descriptors(nblocks, nch=nch, seed=0xD5)
    ch["prn"][:, 2] = 0
    ch["prn"][nblocks // 2:, 4] = 31
    delt = 1.0 / fs
    want, _, hz = oracle.fill_blocks(ch, delt, nsamp, chain=True)
    assert hz["itable_512"] == 0 and hz["dwrd_oob"] == 0
    total = np.zeros(want.shape, np.int64)
    for i in range(nch):
        one = ch.copy()
        one["prn"][:, np.arange(nch) != i] = 0
        one["gain"] = 1.0
        r, _, _ = oracle.fill_blocks(one, delt, nsamp, chain=True)
        if i == 2:
            assert not r.any()
        else:
            assert int(np.abs(r).max()) <= 512
        total += np.trunc(ch["gain"][:, i, None, None] * r.astype(np.float64)).astype(np.int64)
    assert (total.astype(np.int16) == want).all() and int(np.abs(total).max()) < 32768


def test_despread_host_against_a_loop(pkg):
    """despread_host on a small case — a ragged last tile and last segment — for seg_tiles 1, 3 and more than the block holds,
    against the definition written out sample by sample."""
    rng = np.random.default_rng(5)
    nb, nch, nsamp = 2, 3, 5 * 1024 + 37
    u = rng.integers(-32768, 32768, (nb, nsamp, 2))
    r = rng.integers(-512, 513, (nb, nch, nsamp, 2))
    r[:, 1] = 0
    for st in (1, 3, 9):
        got = pkg.despread_host(u, r, st)
        L = 1024 * st
        nseg = -(-nsamp // L)
        assert got.shape == (nb, nch, nseg, 2) and got.dtype == np.int64
        assert nseg == pkg.despread_segments(nsamp, st)
        want = np.zeros((nb, nch, nseg, 2), np.int64)
        for b in range(nb):
            for i in range(nch):
                for j in range(nsamp):
                    ui, uq, c, s = int(u[b, j, 0]), int(u[b, j, 1]), int(r[b, i, j, 0]), int(r[b, i, j, 1])
                    want[b, i, j // L, 0] += ui * c + uq * s
                    want[b, i, j // L, 1] += uq * c - ui * s
        assert (got == want).all(), st
        assert not got[:, 1].any()


def test_view_host(pkg):
    """view_host is apply_noise then the quantiser, unpacked: against pack_iq where that packs, and any nsamp for SC1"""
    rng = np.random.default_rng(6)
    iq = rng.integers(-32768, 32768, (2, 1001, 2)).astype(np.int16)
    nz = pkg.Noise(7, (1 << 34) + 1, 3000.0, 2, 0)
    w, _ = pkg.apply_noise(iq, 7, (1 << 34) + 1, 3000.0, 2)
    assert (pkg.view_host(iq) == iq).all() and (pkg.view_host(iq, pkg.OUT_SC16, nz) == w).all()
    for sh in (0, 5, 15):
        assert (pkg.view_host(iq, pkg.OUT_SC8(sh), nz) == pkg.pack_iq(w, pkg.OUT_SC8(sh))).all()
    v1 = pkg.view_host(iq, pkg.OUT_SC1, nz)
    assert ((v1 == 1) == (w > 0)).all() and ((v1 == -1) == (w <= 0)).all()
    bits = np.unpackbits(pkg.pack_iq(w[:, :1000], pkg.OUT_SC1), axis=-1, bitorder="big").reshape(2, 1000, 2)
    assert ((v1[:, :1000] > 0) == (bits == 1)).all()
    with pytest.raises(ValueError):
        pkg.view_host(iq, 3 << 8)


def test_host_calls_of_the_abi(pkg):
    """gpsbb_despread_segments and gpsbb_cn0_estimate against numpy, strides and the NaN cases included"""
    L = pkg.lib()
    for nsamp, st in ((1, 1), (1024, 1), (1025, 1), (300000, 2), (300000, 293), (300000, 1000), (2500000, 7), ((1 << 31) - 1, 3)):
        assert L.gpsbb_despread_segments(nsamp, st) == -(-nsamp // (1024 * st))
    assert L.gpsbb_despread_segments(0, 1) == -1 and L.gpsbb_despread_segments(100, 0) == -1
    rng = np.random.default_rng(8)
    n, stride = 500, 3
    p = np.zeros((n * stride, 2), np.int64)
    p[:, 0] = rng.normal(4e8, 3e7, n * stride)
    p[:, 1] = rng.normal(0, 3e7, n * stride)
    T = 2048 / 2.6e6
    for st in (1, stride):
        sel = p[::st][:n]
        want = 10 * math.log10(sel[:, 0].mean() ** 2 / (2 * T * sel[:, 1].var(ddof=1)))
        got = L.gpsbb_cn0_estimate(p.ctypes.data, n, st, T)
        assert abs(got - want) < 1e-9, (st, got, want)
    assert abs(pkg.cn0_estimate(p[:n], T) - L.gpsbb_cn0_estimate(p.ctypes.data, n, 1, T)) == 0.0
    one = (Corr * 4)(Corr(10, 3), Corr(12, -3), Corr(9, 1), Corr(11, 0))
    assert math.isfinite(L.gpsbb_cn0_estimate(one, 4, 1, 1e-3))
    assert math.isnan(L.gpsbb_cn0_estimate(one, 1, 1, 1e-3))                      # n < 2
    assert math.isnan(L.gpsbb_cn0_estimate(None, 4, 1, 1e-3))
    assert math.isnan(L.gpsbb_cn0_estimate(one, 4, 0, 1e-3)) and math.isnan(L.gpsbb_cn0_estimate(one, 4, 1, 0.0))
    flat = (Corr * 3)(Corr(10, 5), Corr(12, 5), Corr(9, 5))
    assert math.isnan(L.gpsbb_cn0_estimate(flat, 3, 1, 1e-3))                     # zero variance
    neg = (Corr * 3)(Corr(-10, 5), Corr(-12, 4), Corr(9, 7))
    assert math.isnan(L.gpsbb_cn0_estimate(neg, 3, 1, 1e-3))                      # mean not positive
    assert C.sizeof(Corr) == 16


# ---- the receiver's view, end to end ---------------------------------------------------------------------------------------
# 2.6 MS/s, 300 000-sample blocks, 12 channels of gain 0.3 - 0.8, 10 chained blocks, the library's noise at 45 dB-Hz (shift 0),
# segments of two tiles: 146 whole ones per block, K = 1460.
FS, NSAMP, NCH, NBLOCKS, SEG_TILES, CN0 = 2.6e6, 300000, 12, 10, 2, 45.0
K = NBLOCKS * (NSAMP // (1024 * SEG_TILES))
# three sigma of a variance estimated over K segments (var(s^2) / sigma^4 = 2 / (K - 1)), in dB: derived, not tuned
TOL_DB = 10 * math.log10(1 + 3 * math.sqrt(2.0 / (K - 1)))


def whole(p):
    """[nblocks, nch, nseg, 2] -> [nch, K, 2]: the whole segments of every block, in order"""
    w = p[:, :, :NSAMP // (1024 * SEG_TILES)]
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3).reshape(p.shape[1], -1, 2))


def expected_cn0(pkg, gain, clean_q, sigma):
    """45 + 20 log10(gain) - 10 log10(1 + V_x / (sigma^2 L P1)): V_x the variance the other channels' cross-correlation alone
    leaves in P.q (the noiseless render), sigma^2 L P1 the thermal part"""
    s, c = pkg.sincos_tables()
    p1 = float(np.mean(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2))
    vx = clean_q.astype(np.float64).var(ddof=1)
    return CN0 + 20 * math.log10(gain) - 10 * math.log10(1 + vx / (sigma ** 2 * 1024 * SEG_TILES * p1))


def test_the_cn0_a_receiver_finds(pkg, oracle):
    """SC16: the estimate of every channel within TOL_DB (0.46 dB) of what was asked for, scaled by its gain and less the other
    channels' cross-correlation.  SC8 and SC1: the despreading losses are printed (README quotes them), and only their order is
    asserted: SC1 < SC8 at the right shift <= SC16 + TOL_DB.
    Seen: SC16 residuals -0.44 .. +0.30 dB; losses against SC16: SC8 shift 6 -0.03 .. +0.01 dB, SC8 shift 4 (two too small: it
    clips) -0.86 .. -0.71, SC1 -2.00 .. -1.70 (2 / pi is -1.96)."""
    assert K == 1460 and abs(TOL_DB - 0.46) < 0.005
    delt = 1.0 / FS
    ch = pkg.synth_descriptors(NBLOCKS, nch=NCH, seed=45)
    assert 0.3 <= ch["gain"].min() and ch["gain"].max() <= 0.8
    ch["gain"] = ch["gain"][0]   # a channel keeps its gain over the second
    iq, _, _ = oracle.fill_blocks(ch, delt, NSAMP, chain=True)
    rep = dc.replicas(oracle, ch, delt, NSAMP, chain=True)
    sigma = pkg.noise_sigma(CN0, 1.0, delt)
    nz = pkg.Noise(45, 0, sigma, 0, 0)
    T = 1024 * SEG_TILES * delt
    clean = whole(pkg.despread_host(pkg.view_host(iq), rep, SEG_TILES))
    est = {}
    for name, fmt in (("sc16", pkg.OUT_SC16), ("sc8 shift 6", pkg.OUT_SC8(6)), ("sc8 shift 4", pkg.OUT_SC8(4)), ("sc1", pkg.OUT_SC1)):
        p = whole(pkg.despread_host(pkg.view_host(iq, fmt, nz), rep, SEG_TILES))
        assert p.shape == (NCH, K, 2)
        est[name] = np.array([pkg.cn0_estimate(p[i], T) for i in range(NCH)])
    want = np.array([expected_cn0(pkg, float(ch["gain"][0, i]), clean[i, :, 1], sigma) for i in range(NCH)])
    print("\nPRN gain  asked  sc16   resid | loss sc8>>6  sc8>>4   sc1")
    for i in range(NCH):
        print("%3d %.3f %6.2f %6.2f %+6.2f | %+10.2f %+7.2f %+6.2f" % (
            ch["prn"][0, i], ch["gain"][0, i], want[i], est["sc16"][i], est["sc16"][i] - want[i],
            est["sc8 shift 6"][i] - est["sc16"][i], est["sc8 shift 4"][i] - est["sc16"][i], est["sc1"][i] - est["sc16"][i]))
    resid = est["sc16"] - want
    print("sc16 residuals %+.2f .. %+.2f dB (tolerance %.2f)" % (resid.min(), resid.max(), TOL_DB))
    assert np.isfinite(resid).all() and (np.abs(resid) <= TOL_DB).all(), resid
    assert (est["sc1"] < est["sc8 shift 6"]).all()
    assert (est["sc8 shift 6"] <= est["sc16"] + TOL_DB).all()
