"""Despreading at lags on the CPU: despread_lags_host (the numpy restatement of gpsbb_batch_despread_lags) against despread_host
and against the definition, and what it is for — the receiver's view of a multipath echo from the front end, a second peak of
the correlation function where the echo's delay says.  No GPU is touched."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_lags_check as dlc  # noqa: E402


def random_case(seed, nb=2, nch=3, nsamp=2 * 1024 + 37):
    rng = np.random.default_rng(seed)
    u = rng.integers(-32768, 32768, (nb, nsamp, 2))
    r = rng.integers(-512, 513, (nb, nch, nsamp, 2))
    r[:, 1] = 0
    return u, r


def test_lag_0_is_despread_host(pkg):
    u, r = random_case(1)
    for st in (1, 2, 7):
        got = pkg.despread_lags_host(u, r, st, (3, 0, -2, 0))
        want = pkg.despread_host(u, r, st)
        assert got.shape == want.shape[:3] + (4, 2) and got.dtype == np.int64
        assert (got[:, :, :, 1] == want).all() and (got[:, :, :, 3] == want).all()
        assert (pkg.despread_lags_host(u, r, st, [0])[:, :, :, 0] == want).all()


def test_against_the_definition_at_both_block_edges(pkg):
    """P(L) = sum_n w[n + L] * conj(r[n]) over the samples n of a segment, a term whose n + L falls outside [0, nsamp) zero:
    written out with explicit slices, for lags that reach past either edge, past a tile and past the whole (short) block."""
    for nsamp, lags in ((2 * 1024 + 37, (-64, -1, 0, 1, 64, 5, 5)), (40, (-64, -39, -1, 0, 1, 39, 64, 40))):
        u, r = random_case(nsamp, nsamp=nsamp)
        for st in (1, 3):
            got = pkg.despread_lags_host(u, r, st, lags)
            seg = 1024 * st
            for k, lag in enumerate(lags):
                for s in range(-(-nsamp // seg)):
                    n = np.arange(s * seg, min((s + 1) * seg, nsamp))
                    n = n[(n + lag >= 0) & (n + lag < nsamp)]
                    wi, wq = u[:, None, n + lag, 0], u[:, None, n + lag, 1]
                    c, sn = r[:, :, n, 0], r[:, :, n, 1]
                    assert (got[:, :, s, k, 0] == (wi * c + wq * sn).sum(axis=-1)).all(), (nsamp, st, lag, s)
                    assert (got[:, :, s, k, 1] == (wq * c - wi * sn).sum(axis=-1)).all(), (nsamp, st, lag, s)
            if nsamp == 40:   # a lag as long as the block or longer: nothing; one short of it: a single term
                assert not got[:, :, :, 0].any() and not got[:, :, :, 6].any() and not got[:, :, :, 7].any()
                assert (got[:, :, 0, 1, 0] == u[:, None, 0, 0] * r[:, :, 39, 0] + u[:, None, 0, 1] * r[:, :, 39, 1]).all()
                assert (got[:, :, 0, 5, 0] == u[:, None, 39, 0] * r[:, :, 0, 0] + u[:, None, 39, 1] * r[:, :, 0, 1]).all()


def test_a_shifted_copy_of_a_replica_peaks_at_its_shift(pkg):
    """u[n] = r[n - D]: the sum at lag D is sum |r|^2 over the samples that have a partner, and no other lag comes near it"""
    rng = np.random.default_rng(7)
    nsamp = 3 * 1024 + 37
    r = rng.choice([-250, 250], (1, 1, nsamp, 2))
    lags = list(range(-8, 9))
    for d in (5, -3, 0):
        u = np.zeros((1, nsamp, 2), np.int64)
        if d >= 0:
            u[0, d:] = r[0, 0, :nsamp - d]
        else:
            u[0, :nsamp + d] = r[0, 0, -d:]
        p = pkg.despread_lags_host(u, r, 4, lags)[0, 0, 0]
        mag = np.hypot(p[:, 0], p[:, 1])
        assert lags[int(np.argmax(mag))] == d
        assert p[lags.index(d), 0] == 2 * 250 * 250 * (nsamp - abs(d)) and p[lags.index(d), 1] == 0
        assert np.sort(mag)[-2] < 0.1 * mag.max()


def test_the_receivers_view_of_an_echo(pkg, oracle):
    """One block of 0.1 s at 2.6 MS/s of the golden scenario, the satellite of slot 0 with an echo three samples late
    (extra_m = 3 c / fs) and 6 dB down.  The lag profile of the render with the echo less the profile of the render without it
    is the echo's own (the render is a sum of per-channel truncations: tests/test_echo.py, so the subtraction is exact): against
    the direct channel's replica its largest magnitude over lags -4 .. 8 is at L = 3, and that magnitude over the |P(0)| of the
    direct channel's own contribution (the render of that channel alone, so that neither side holds another satellite's
    cross-correlation) is 10^(-6/20) within 2 / (alpha * gain * 512) + 1e-3: the first term is what truncation towards zero can
    take from an amplitude of alpha * gain * 250 and less (a unit per component, against the direct channel's smaller relative
    loss), with gain read from the descriptor; the second covers the carrier table's 512 steps (the echo's phase differs by a
    constant, its index is rounded down at other samples) and the handful of samples whose chips differ at three samples'
    distance."""
    fs, nsamp = 2.6e6, 260000
    ch, prn = dlc.echo_descriptors(pkg, 1, fs, max_chan=12, idle=None)
    assert ch.shape == (1, 13)
    delt = 1.0 / fs
    alone = ch.copy()
    alone["prn"][:, 1:] = 0
    without = ch.copy()
    without["prn"][:, 12] = 0
    rep = dlc.dc.replicas(oracle, alone, delt, nsamp)[:, :1]
    lags = list(range(-4, 9))

    def profile(d):
        return pkg.despread_lags_host(pkg.view_host(oracle.fill_blocks(d, delt, nsamp)[0]), rep, 1 << 20, lags)[0, 0, 0]

    echo = profile(ch) - profile(without)
    mag = np.hypot(echo[:, 0].astype(np.float64), echo[:, 1].astype(np.float64))
    p0 = profile(alone)[lags.index(0)]
    ratio = mag.max() / np.hypot(float(p0[0]), float(p0[1]))
    alpha, gain = 10.0 ** (-6.0 / 20.0), float(ch["gain"][0, 0])
    assert ch["gain"][0, 12] == gain * alpha
    tol = 2.0 / (alpha * gain * 512.0) + 1e-3
    print("echo peak at lag %d, |P(3)| / |P_direct(0)| = %.5f against %.5f (tolerance %.5f, gain %.4f)"
          % (lags[int(np.argmax(mag))], ratio, alpha, tol, gain))
    assert lags[int(np.argmax(mag))] == 3
    assert abs(ratio - alpha) <= tol
