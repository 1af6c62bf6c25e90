"""Receiver noise (include/gpsbb.h gpsbb_noise_t) on the CPU: the numpy restatement the GPU is checked against — Philox4x32-10 on
the Random123 known answers, position addressing, the statistics of the deviates, the knot table against the exact normal
quantile — gpsbb_noise_sigma against the worked table, apply_noise on hand-worked values, and gpsbb-sim's refusal of a bad -W.
No GPU is touched."""
import math
import os
import statistics
import subprocess

import numpy as np
import pytest

ND = statistics.NormalDist()


@pytest.fixture(scope="module")
def table(pkg):
    return pkg.noise_table()


def knot_t(i):
    """the t of knot i (include/gpsbb.h step 2)"""
    if i < 128:
        return i
    e = i // 64 + 5
    return (1 << e) + (i % 64) * (1 << (e - 6))


def exact_q16(t):
    """2^16 * Phi^-1(1 - (t + 0.5) / 2^32), in double precision"""
    return 65536.0 * ND.inv_cdf(1.0 - (t + 0.5) / 2.0 ** 32)


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(pkg, ctr, key, want):
    got = pkg.philox4x32_10(np.array([ctr], np.uint64), key)
    assert got.dtype == np.uint32 and got.shape == (1, 4)
    assert tuple(int(x) for x in got[0]) == want


def test_philox_words_are_the_samples_of_a_pair(pkg, table):
    """u = x[2 * (s & 1) + c] of the call with counter s >> 1: sample 2m takes words 0, 1 and sample 2m + 1 words 2, 3"""
    seed = 0x0123456789ABCDEF
    x = pkg.philox4x32_10(np.array([[3, 0, 0, 0]], np.uint64), (seed & 0xFFFFFFFF, seed >> 32))[0]
    z = pkg.noise_z(x, table)
    s256 = 256 * 1000
    want = [(s256 * int(v) + (1 << 23)) >> 24 for v in z]
    got = pkg.noise_host(seed, 6, 2, 1000.0, table)
    assert got.ravel().tolist() == want


# ---- position addressing --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 1, 2, 7, 1000, 1001, 65535])
def test_noise_host_is_position_addressed(pkg, table, k):
    whole = pkg.noise_host(7, 0, 70000, 2500.0, table)
    part = pkg.noise_host(7, k, 3001, 2500.0, table)
    assert part.dtype == np.int32 and part.shape == (3001, 2)
    assert (part == whole[k:k + 3001]).all()


def test_noise_host_far_positions_and_seeds(pkg, table):
    """positions beyond 2^32 pairs use the high counter word; the seed's high half is the second key word"""
    s0 = (1 << 33) + 5
    a = pkg.noise_host(1, s0, 64, 1000.0, table)
    b = pkg.noise_host(1, s0 & 0xFFFFFFFF, 64, 1000.0, table)
    assert (a != b).any()
    assert (pkg.noise_host((1 << 32) | 1, 0, 64, 1000.0, table) != pkg.noise_host(1, 0, 64, 1000.0, table)).any()
    assert (pkg.noise_host(1, s0 + 3, 10, 1000.0, table) == a[3:13]).all()


# ---- statistics over 2^22 samples at sigma = 1000 ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def big(pkg, table):
    return pkg.noise_host(1, 0, 1 << 22, 1000.0, table).astype(np.float64)


def test_noise_moments(big):
    x = big.ravel()
    sigma2 = 1000.0 ** 2 + 1.0 / 12.0
    assert abs(x.mean()) <= 1.5
    v = x.var()
    assert abs(v / sigma2 - 1.0) <= 0.003, v
    kurt = ((x - x.mean()) ** 4).mean() / v ** 2 - 3.0
    assert abs(kurt) <= 0.01, kurt


def test_noise_tails(big):
    x = np.abs(big.ravel()) / 1000.0
    for k, tol in ((3.0, 0.05), (4.0, 0.15)):
        want = 2.0 * (1.0 - ND.cdf(k))
        got = float(np.count_nonzero(x > k)) / x.size
        assert abs(got / want - 1.0) <= tol, (k, got, want)


def test_noise_ks_distance(big):
    """the integer deviates against N(0, 1000) at every value they take, continuity-corrected"""
    vals, counts = np.unique(big.ravel().astype(np.int64), return_counts=True)
    emp = np.cumsum(counts) / counts.sum()
    nd = statistics.NormalDist(0.0, 1000.0)
    ref = np.array([nd.cdf(v + 0.5) for v in vals.tolist()])
    d = float(np.max(np.abs(emp - ref)))
    assert d <= 1e-3, d


def test_noise_is_white_and_independent(pkg, table, big):
    n = big.shape[0]
    bound = 5.0 / math.sqrt(n)
    i = big[:, 0] - big[:, 0].mean()
    q = big[:, 1] - big[:, 1].mean()
    vi, vq = (i * i).mean(), (q * q).mean()
    for lag in range(1, 17):
        for a, va in ((i, vi), (q, vq)):
            r = (a[lag:] * a[:-lag]).mean() / va
            assert abs(r) <= bound, (lag, r)
    for lag in range(0, 17):
        r = (i[lag:] * q[:n - lag]).mean() / math.sqrt(vi * vq)
        assert abs(r) <= bound, (lag, r)
        r = (q[lag:] * i[:n - lag]).mean() / math.sqrt(vi * vq)
        assert abs(r) <= bound, (lag, r)
    other = pkg.noise_host(2, 0, n, 1000.0, table).astype(np.float64)
    for c in (0, 1):
        a, b = big[:, c] - big[:, c].mean(), other[:, c] - other[:, c].mean()
        r = (a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean())
        assert abs(r) <= bound, (c, r)


# ---- the knot table and G(u) ------------------------------------------------------------------------------------------

def test_noise_table_knots(pkg, table):
    assert table.dtype == np.int32 and table.size == pkg.NOISE_KNOTS == 1665
    assert pkg.lib().gpsbb_noise_table(None, 0) == 1665
    for i in range(table.size):
        t = knot_t(i)
        assert abs(int(table[i]) - exact_q16(t)) <= 1.0, (i, t)
    assert (np.diff(table.astype(np.int64)) <= 0).all()     # |z| falls as t rises
    assert table[0] / 65536.0 >= 6.3
    assert table[-1] == 0                                    # t = 2^31: the median


def test_noise_deviate_against_the_exact_quantile(pkg, table):
    rng = np.random.default_rng(11)
    u = np.concatenate([rng.integers(0, 1 << 32, size=100000, dtype=np.uint64),
                        np.uint64(0x7FFFFFFF) - np.arange(4096, dtype=np.uint64),        # every t < 4096, positive
                        np.uint64(0xFFFFFFFF) - np.arange(4096, dtype=np.uint64)])       # ... and negative
    z = pkg.noise_z(u, table)
    t = (0x7FFFFFFF - (u & np.uint64(0x7FFFFFFF)).astype(np.int64))
    sign = np.where((u >> np.uint64(31)) != 0, -1.0, 1.0)
    exact = sign * np.array([exact_q16(int(v)) for v in t.tolist()])
    err = np.abs(z - exact)
    assert float(err.max()) <= 5e-5 * 65536 + 1.0, float(err.max())


# ---- sigma ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,want", [(2.6e6, (5819, 3272, 1840)), (25e6, (18045, 10147, 5706))])
def test_noise_sigma_worked_table(pkg, fs, want):
    for cn0, w in zip((40, 45, 50), want):
        assert abs(pkg.noise_sigma(cn0, 1.0, 1.0 / fs) - w) <= 0.5, (fs, cn0)
    # sigma scales with the gain and with the square root of the rate
    assert abs(pkg.noise_sigma(45, 2.0, 1.0 / fs) / pkg.noise_sigma(45, 1.0, 1.0 / fs) - 2.0) < 1e-12


def test_noise_sigma_refuses_non_finite(pkg):
    for args in ((float("nan"), 1.0, 1e-6), (float("inf"), 1.0, 1e-6), (45.0, 0.0, 1e-6), (45.0, 1.0, 0.0), (45.0, 1.0, float("nan"))):
        assert math.isnan(pkg.noise_sigma(*args)), args


# ---- apply_noise ------------------------------------------------------------------------------------------------------

V = [-32768, -32767, -17, -16, -1, 0, 1, 15, 16, 4095, 4096, 32766, 32767, 100]


def test_apply_noise_without_noise_is_the_shift(pkg, table):
    """sigma = 1/1024 rounds to S = 0: N = 0 everywhere, w = v >> shift (a floor)"""
    iq = np.array(V, np.int16).reshape(-1, 2)
    for shift in range(8):
        w, n = pkg.apply_noise(iq, 5, 0, 1.0 / 1024, shift, table)
        assert w.dtype == np.int16 and w.shape == iq.shape and n == 0
        assert w.ravel().tolist() == [v // (1 << shift) for v in V], shift
    assert pkg.apply_noise(iq, 5, 0, 1.0 / 1024, 3, table)[0].ravel().tolist()[:4] == [-4096, -4096, -3, -2]


def test_apply_noise_saturates_at_both_ends(pkg, table):
    nz = pkg.noise_host(9, 100, 64, 30000.0, table).astype(np.int64)
    pos = [k for k in range(128) if nz.ravel()[k] > 0]
    neg = [k for k in range(128) if nz.ravel()[k] < 0]
    v = np.zeros(128, np.int64)
    v[pos] = 32767
    v[neg] = -32768
    iq = v.astype(np.int16).reshape(64, 2)
    w, n = pkg.apply_noise(iq, 9, 100, 30000.0, 0, table)
    assert (w.ravel()[pos] == 32767).all() and (w.ravel()[neg] == -32768).all()
    assert n == len(pos) + len(neg)
    # by hand for each shift: sat16((v + N) >> shift)
    for shift in range(8):
        w, n = pkg.apply_noise(iq, 9, 100, 30000.0, shift, table)
        want = [max(-32768, min(32767, (int(a) + int(b)) >> shift)) for a, b in zip(v, nz.ravel())]
        raw = [(int(a) + int(b)) >> shift for a, b in zip(v, nz.ravel())]
        assert w.ravel().tolist() == want, shift
        assert n == sum(1 for a, b in zip(raw, want) if a != b), shift
    assert n == 0   # shift 7 leaves room for +-32767 + 6.34 sigma


def test_apply_noise_then_sc1_of_a_shifted_value(pkg, table):
    """SC1 packs the sign of the noisy, shifted value: a small v whose noise flips it flips the bit"""
    nz = pkg.noise_host(3, 0, 8, 500.0, table).astype(np.int64).ravel()
    v = np.where(nz > 0, -1, 1).astype(np.int16)              # each component's noise outweighs its sign
    w, _ = pkg.apply_noise(v.reshape(8, 2), 3, 0, 500.0, 2, table)
    bits = [1 if ((int(a) + int(b)) >> 2) > 0 else 0 for a, b in zip(v, nz)]
    want = [int("".join(map(str, bits[8 * m:8 * m + 8])), 2) for m in range(2)]
    assert pkg.pack_iq(w, pkg.OUT_SC1).tolist() == want
    assert pkg.pack_iq(v.reshape(8, 2), pkg.OUT_SC1).tolist() != want


def test_apply_noise_blocks_are_one_stream(pkg, table):
    rng = np.random.default_rng(4)
    iq = rng.integers(-3000, 3000, size=(3, 101, 2)).astype(np.int16)
    w, n = pkg.apply_noise(iq, 77, 13, 800.0, 1, table)
    for b in range(3):
        wb, _ = pkg.apply_noise(iq[b], 77, 13 + 101 * b, 800.0, 1, table)
        assert (w[b] == wb).all()


# ---- gpsbb-sim --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arg", ["nan", "inf", "-inf", "abc", "45,8", "45,-1", "45,1x", "45x", ""])
def test_gpsbb_sim_refuses_a_bad_noise_option(pkg, tmp_path, arg):
    """-W cn0[,shift]: a C/N0 that is not finite or a shift outside 0..7 is refused before a GPU or a file is touched"""
    pkg.build_frontend()
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    out = tmp_path / "never.bin"
    r = subprocess.run([exe, "-e", "/nonexistent.14n", "-W", arg, "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "-W" in r.stderr
    assert not out.exists()
