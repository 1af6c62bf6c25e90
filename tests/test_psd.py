"""The power spectrum without a GPU: the numpy mirror psd_host against a term-by-term restatement in Python integers and against
np.fft on the same windowed segments (dynamic range, the sum of the bins), the twiddle table's identities, the split property,
gpsbb_psd_make's defaults, windows and refusals, gpsbb_psd_min_shift on both sides of the rule, and tools/psd_asan.cpp built and
run under the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import psd_check as pc  # noqa: E402

BADARG = -1


def brute(w, psd):
    """the definition once more, a butterfly at a time in Python integers"""
    tc, ts = [[int(v) for v in t] for t in __import__("pluto_gps_sim_amd").psd_twiddles()]
    L, hop, shift = int(psd.log2n), int(psd.hop), int(psd.shift)
    N = 1 << L
    win = [int(v) for v in psd.window()]
    nseg = (len(w) - N) // hop + 1
    out = [0] * N
    for sg in range(nseg):
        a = [None] * N
        for n in range(N):
            r = int(format(n, "0%db" % L)[::-1], 2)
            a[r] = [(int(w[sg * hop + n][c]) * win[n]) >> 1 for c in range(2)]
        m = 2
        while m <= N:
            h = m // 2
            for j0 in range(0, N, m):
                for j in range(h):
                    c, s = tc[j * (4096 // m)], ts[j * (4096 // m)]
                    u, v = a[j0 + j], a[j0 + j + h]
                    t = [(v[0] * c + v[1] * s + (1 << 29)) >> 30, (v[1] * c - v[0] * s + (1 << 29)) >> 30]
                    assert all(abs(u[k] + t[k]) < 1 << 31 and abs(u[k] - t[k]) < 1 << 31 for k in range(2))
                    a[j0 + j], a[j0 + j + h] = [(u[k] + t[k] + 1) >> 1 for k in range(2)], [(u[k] - t[k] + 1) >> 1 for k in range(2)]
            m *= 2
        for k in range(N):
            out[k] += (a[k][0] >> shift) ** 2 + (a[k][1] >> shift) ** 2
    return out, nseg


def test_mirror_term_by_term(pkg):
    """N = 64, two segments, a random window with -32768 in it, full-range samples: == in Python integers"""
    iq = pc.ac.random_iq(64 + 37, 0x951)
    for shift in (0, 3):
        p = pkg.Psd(6, 37, shift, pc.random_window(64, 0x952))
        got, nseg = pkg.psd_host(iq, p)
        want, wn = brute(iq.tolist(), p)
        assert nseg == wn == 2 and [int(v) for v in got] == want


def tone(amp, f, n):
    t = np.arange(n)
    return np.stack([np.rint(amp * np.cos(2 * np.pi * f * t)), np.rint(amp * np.sin(2 * np.pi * f * t))], 1).astype(np.int16)


@pytest.mark.parametrize("amp", [20000, 1000, 50])
def test_dynamic_range_follows_fft(pkg, amp):
    """an off-bin tone under Hann at N = 1024, the seven segments shift 0 serves: the tone's bin over the mean of the far floor is
    within 0.5 dB of the same figure from np.fft on the same windowed segments — the integers' rounding floor lies below the
    tone's own quantisation floor (108.75, 95.52 and 69.54 dB, the same to 0.01 dB)."""
    N = 1024
    w = tone(amp, 100.3 / N, 4 * N)
    p = pkg.psd_make(10, w.shape[0], 0, pkg.PSD_HANN)
    assert (p.hop, p.shift) == (N // 2, 0)
    got, nseg = pkg.psd_host(w, p)
    assert nseg == 7
    win = p.window().astype(np.float64)
    idx = np.arange(nseg)[:, None] * int(p.hop) + np.arange(N)[None, :]
    z = (w[:, 0].astype(np.float64) + 1j * w[:, 1])[idx] * win[None, :]
    pf = (np.abs(np.fft.fft(z, axis=1)) ** 2).sum(0)
    k = int(np.argmax(got))
    assert k == int(np.argmax(pf)) == 100
    db = 10 * np.log10(float(got[k]) / got[k + 20:k + 500].astype(np.float64).mean())
    db_f = 10 * np.log10(pf[k] / pf[k + 20:k + 500].mean())
    print("amplitude %d: tone over far floor %.2f dB, np.fft %.2f dB" % (amp, db, db_f))
    assert abs(db - db_f) <= 0.5


@pytest.mark.parametrize("log2n,amp", [(6, 30000), (10, 3000), (12, 300), (10, 20)])
def test_sum_of_bins_is_the_mean_square(pkg, log2n, amp):
    """Gaussian int16 under the rectangular window: sum(psd) * psd_scale within 1e-4 of the exact mean square, at the plan's own
    shift and four above it"""
    N = 1 << log2n
    rng = np.random.default_rng(log2n * 1000 + amp)
    w = np.clip(np.rint(rng.standard_normal((8 * N, 2)) * amp / 3), -32768, 32767).astype(np.int16)
    exact = float((w.astype(np.int64) ** 2).sum()) / w.shape[0]
    p = pkg.psd_make(log2n, w.shape[0])
    assert (p.hop, p.shift) == (N, 1)
    for shift in (1, 4):
        q = p.copy(shift=shift)
        got, nseg = pkg.psd_host(w, q)
        est = float(got.astype(np.float64).sum()) * pkg.psd_scale(q, nseg)
        print("N %d amplitude %d shift %d: %.3e" % (N, amp, shift, est / exact - 1))
        assert nseg == 8 and abs(est / exact - 1) <= 1e-4


def test_views_fill_the_same_range(pkg):
    """SC8 and SC1 samples at the end of their range give the bins SC16's give at the end of its own; psd_scale differs by 4^Wbits"""
    p = pkg.Psd(7, 128, 0, np.full(128, -32768, np.int16))
    a, _ = pkg.psd_host(np.full((256, 2), -32768), p, pkg.OUT_SC16)
    b, _ = pkg.psd_host(np.full((256, 2), -128), p, pkg.OUT_SC8(3))
    c, _ = pkg.psd_host(np.full((256, 2), -1), p, pkg.OUT_SC1)
    assert (a == b).all() and (a == c).all() and int(a[0]) == 2 * 2 << 58 and not a[1:].any()
    s16, s8, s1 = (pkg.psd_scale(p, 2, v) for v in (pkg.OUT_SC16, pkg.OUT_SC8(3), pkg.OUT_SC1))
    assert s16 / s8 == 4.0 ** 8 and s8 / s1 == 4.0 ** 7
    assert abs(float(a.sum()) * s16 / (2 * 32768.0 ** 2) - 1) < 1e-12 and abs(float(c.sum()) * s1 / 2.0 - 1) < 1e-12


def test_twiddle_table(pkg):
    c, s = pkg.psd_twiddles()
    k = np.arange(2048)
    assert c[0] == 1 << 30 and s[0] == 0 and c[1024] == 0 and s[1024] == 1 << 30
    assert (c[2048 - k[1:]] == -c[1:]).all() and (s[2048 - k[1:]] == s[1:]).all() and (c[:1025] == s[1024 - k[:1025]]).all()
    assert np.abs(c - np.rint(np.ldexp(np.cos(2 * np.pi * k / 4096), 30))).max() <= 1
    assert np.abs(s - np.rint(np.ldexp(np.sin(2 * np.pi * k / 4096), 30))).max() <= 1
    assert pkg.lib().gpsbb_psd_twiddles(None, None) == BADARG


def test_split_on_the_mirror(pkg):
    """the spectrum of a buffer == the bin-wise sum of the spectra of the first k segments and of the rest, at the same shift"""
    N, hop = 256, 100
    iq = pc.ac.random_iq(N + 20 * hop + 9, 0x953)
    p = pkg.Psd(8, hop, pkg.psd_min_shift(21), pc.random_window(N, 0x954))
    whole, nseg = pkg.psd_host(iq, p)
    assert nseg == 21
    for k in (1, 8, 20):
        a, na = pkg.psd_host(iq[:N + (k - 1) * hop], p)
        b, nb = pkg.psd_host(iq[k * hop:], p)
        assert (na, nb) == (k, 21 - k) and (a + b == whole).all()


def test_psd_make(pkg):
    L = pkg.lib()
    for log2n in range(pkg.PSD_MIN_LOG2N, pkg.PSD_MAX_LOG2N + 1):
        N = 1 << log2n
        r = pkg.psd_make(log2n, 9 * N)
        assert (r.log2n, r.hop, r.shift) == (log2n, N, 1) and (r.window() == 16384).all() and not np.frombuffer(r.win, np.int16)[N:].any()
        h = pkg.psd_make(log2n, 4 * N, 0, pkg.PSD_HANN)
        w = h.window()
        assert (h.hop, h.shift) == (N // 2, 0) and w[0] == 0 and w[N // 2] == 16384 and (w[1:] == w[1:][::-1]).all()
        assert np.abs(w - np.rint(16384 * 0.5 * (1 - np.cos(2 * np.pi * np.arange(N) / N)))).max() <= 1
        assert pkg.psd_make(log2n, 4 * N, 7, pkg.PSD_HANN).hop == 7
        assert pkg.psd_make(log2n, N + 1000 * 3, 3).shift == pkg.psd_min_shift(1001)
    p = pkg.Psd(6, 5, 3, [7] * 64)
    keep = bytes(p)
    for args in ((5, 0, 0, 1 << 20), (13, 0, 0, 1 << 20), (6, 0, 2, 64), (6, 0, -1, 64), (6, 0, 0, 63), (6, (1 << 20) + 1, 0, 1 << 22),
                 (6, 1, 0, 64 + (1 << 20)), (12, 0, 1, 4095)):
        assert L.gpsbb_psd_make(C.byref(p), *args) == BADARG and bytes(p) == keep, args
    assert L.gpsbb_psd_make(None, 6, 0, 0, 64) == BADARG
    for args in ((6, 0, 0, 64), (12, 0, 1, 4096), (6, 1 << 20, 0, 64), (6, 1, 0, 64 + (1 << 20) - 1)):
        assert L.gpsbb_psd_make(C.byref(p), *args) == 0, args
    assert C.sizeof(pkg.Psd) == 8208
    assert all(pkg.exp_lib().gpsbb_test_psd_run(n) == pkg.psd_run(n) for n in range(6, 13)) and pkg.exp_lib().gpsbb_test_psd_run(5) == -1
    assert np.isnan(pkg.psd_scale(pkg.Psd(6, 64, 0, [0] * 64), 1)) and np.isnan(pkg.psd_scale(p, 0)) and np.isnan(pkg.psd_scale(p, 1, 0x300))


def test_min_shift_both_sides(pkg):
    L = pkg.lib()
    assert pkg.psd_min_shift(7) == 0 and pkg.psd_min_shift(8) == 1 and pkg.psd_min_shift(1) == 0
    for nseg in (1, 7, 8, 31, 32, 1000, 1 << 20):
        s = pkg.psd_min_shift(nseg)
        fits = lambda sh: nseg * 2 * (((1 << 30) >> sh) + 1) ** 2 < 1 << 64   # noqa: E731
        assert fits(s) and (s == 0 or not fits(s - 1))
    assert L.gpsbb_psd_min_shift(0) == BADARG and L.gpsbb_psd_min_shift(-3) == BADARG and L.gpsbb_psd_min_shift((1 << 20) + 1) == BADARG
    with pytest.raises(ValueError):
        pkg.psd_host(np.zeros((64 * 8, 2), np.int16), pkg.Psd(6, 64, 0, [1] * 64))
    pkg.psd_host(np.zeros((64 * 8, 2), np.int16), pkg.Psd(6, 64, 1, [1] * 64))


def test_e2e_figures_on_the_mirror(pkg):
    """the end-to-end cases of the GPU test on the CPU oracle's render: the figures they assert hold before any GPU is asked"""
    bad = pc.e2e_cpu(pkg)
    assert not bad, "\n".join(bad)


def test_psd_asan(tmp_path):
    """tools/psd_asan.cpp under -fsanitize=address,undefined: a stand-alone program on the CPU, exit status 0"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "psd_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "pluto-gps-sim_amd", "csrc"), os.path.join(ROOT, "tools", "psd_asan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr):
        pytest.skip("%s cannot link the sanitizer runtimes" % cxx)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "clean" in run.stdout
