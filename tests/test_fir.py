"""The front-end filter without a GPU: gpsbb_fir_make's taps against numpy's own Kaiser window and sinc and against the figures a
design of that kind must reach, the numpy mirror fir_host against a brute-force double loop and its own contract (identity,
constants, one call equals any split), every refusal of gpsbb_fir_make, and tools/fir_asan.cpp built and run under the host
sanitizers."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fir_check as fc  # noqa: E402

BADARG = -1


@pytest.mark.parametrize("T,D", [(33, 4), (65, 8)])
def test_tap_design(pkg, T, D):
    """C taps within 1 of the numpy design per tap (a tie, or a last bit of I0), the sum exactly 2^shift, symmetric; from the taps
    alone: at most -58 dB beyond fc + df / 2 with df = (A - 7.95) / (14.36 (T - 1)), ripple at most 0.03 dB up to fc - df / 2"""
    f = pkg.fir_make(T, D, 0.8, 60.0)
    h = f.taps()
    want = np.rint(fc.design_numpy(T, D, 0.8, 60.0) * (2.0 ** f.shift / 32768.0)).astype(np.int64)
    want[(T - 1) // 2] += (1 << f.shift) - want.sum()
    assert (f.ntaps, f.decim, f.shift) == (T, D, 15) and np.abs(h - want).max() <= 1
    assert h.sum() == 1 << f.shift and (h == h[::-1]).all()
    fcut, df = 0.8 * 0.5 / D, (60.0 - 7.95) / (14.36 * (T - 1))
    fr, db = fc.response_db(f)
    stop, ripple = db[fr >= fcut + df / 2].max(), np.abs(db[fr <= fcut - df / 2]).max()
    print("(%d, %d): stopband %.2f dB, ripple %.4f dB" % (T, D, stop, ripple))
    assert stop <= -58.0 and ripple <= 0.03


def test_taps_closed_form(pkg):
    one = pkg.fir_make(1, 1)
    assert (one.ntaps, one.decim, one.shift, one.taps().tolist()) == (1, 1, 14, [16384])
    assert int(np.abs(pkg.fir_make(33, 4, 0.8, 60.0).taps()).sum()) == 42648
    assert int(np.abs(pkg.fir_make(129, 8, 0.8, 50.0).taps()).sum()) == 53664
    assert bytes(pkg.fir_make(33, 4)) == bytes(pkg.fir_make(33, 4, 0.8, 60.0)) == bytes(pkg.fir_make(33, 4, -1.0, -2.0))
    assert C.sizeof(pkg.Fir) == 276 and pkg.exp_lib().gpsbb_test_fir_tile() == pkg.FIR_TILE


def brute(w, fir, hist):
    T, D, s = fir.ntaps, fir.decim, fir.shift
    h = [int(v) for v in fir.taps()]
    x = ([[0, 0]] * (T - 1) if hist is None else [[int(a), int(b)] for a, b in hist]) + [[int(a), int(b)] for a, b in w]
    y, clips = [], 0
    for m in range(len(w) // D):
        row = []
        for c in range(2):
            acc = sum(h[k] * x[T - 1 + m * D + D - 1 - k][c] for k in range(T))
            r = (acc + (1 << (s - 1))) >> s if s else acc
            v = min(max(r, -32768), 32767)
            clips += v != r
            row.append(v)
        y.append(row)
    return np.array(y, np.int16).reshape(-1, 2), np.array(x[len(x) - (T - 1):], np.int16).reshape(-1, 2), clips


@pytest.mark.parametrize("T,D,shift", [(1, 1, 0), (2, 1, 1), (5, 3, 15), (33, 4, 15), (64, 7, 16), (129, 16, 14)])
def test_fir_host_brute_force(pkg, T, D, shift):
    fir = fc.random_fir(pkg, T, D, shift, 7 * T + D, budget=65535 if shift else 3)
    w = fc.ac.random_iq(max(11 * D, 5), 0xF0 + T)[:11 * D]
    for hist in (None, fc.random_hist(T, 0xF5)):
        got, want = pkg.fir_host(w, fir, hist), brute(w, fir, hist)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[2] == want[2]


def test_fir_host_contract(pkg):
    w = fc.ac.random_iq(600, 0xF6)
    # identity for T = 1
    for fir in (pkg.Fir([1], 1, 0), pkg.fir_make(1, 1)):
        y, hist, clipped = pkg.fir_host(w, fir)
        assert (y == w).all() and hist.shape == (0, 2) and clipped == 0
    # a constant input with a constant history gives the constant: the DC gain is exactly one
    fir = pkg.fir_make(33, 4)
    for v in (-32768, 32767, 12345):
        y, hist, clipped = pkg.fir_host(np.full((40, 2), v, np.int16), fir, np.full((32, 2), v, np.int16))
        assert (y == v).all() and (hist == v).all() and clipped == 0
    # one call == a split at multiples of D, a piece shorter than T - 1 among them
    whole = pkg.fir_host(w, fir)
    parts, hist, clips, at = [], None, 0, 0
    for n in (4, 200, 8, 388):
        y, hist, c = pkg.fir_host(w[at:at + n], fir, hist)
        parts.append(y)
        clips += c
        at += n
    assert at == 600 and (np.concatenate(parts) == whole[0]).all() and (hist == whole[1]).all() and clips == whole[2]
    # a buffer shorter than the history: part of hist_in survives
    h0 = fc.random_hist(33, 0xF7)
    _, h1, _ = pkg.fir_host(w[:8], fir, h0)
    assert (h1[:24] == h0[8:]).all() and (h1[24:] == w[:8]).all()


def test_fir_make_refusals(pkg):
    L = pkg.lib()
    f = pkg.Fir([7], 1, 3)
    keep = bytes(f)
    nan, inf = float("nan"), float("inf")
    for args in ((0, 4, 0.8, 60.0), (-1, 4, 0.8, 60.0), (pkg.FIR_MAX_TAPS + 1, 4, 0.8, 60.0), (33, 0, 0.8, 60.0), (33, 17, 0.8, 60.0),
                 (33, 4, 1.0000001, 60.0), (33, 4, nan, 60.0), (33, 4, 0.8, nan), (33, 4, inf, 60.0), (33, 4, 0.8, inf), (33, 4, -inf, 60.0),
                 (33, 4, 0.8, 180.5)):
        assert L.gpsbb_fir_make(C.byref(f), *args) == BADARG and bytes(f) == keep, args
    assert L.gpsbb_fir_make(None, 33, 4, 0.8, 60.0) == BADARG
    # the served neighbours
    for args in ((1, 4, 0.8, 60.0), (pkg.FIR_MAX_TAPS, 16, 1.0, 180.0), (33, 1, 0.8, 60.0), (33, 16, 0.8, 60.0), (33, 4, 1.0, 60.0), (33, 4, 1e-3, 1.0)):
        assert L.gpsbb_fir_make(C.byref(f), *args) == 0, args
        assert int(np.abs(f.taps()).sum()) <= pkg.FIR_MAX_SUM and f.taps().sum() == 1 << f.shift


def test_fir_asan(tmp_path):
    """tools/fir_asan.cpp under -fsanitize=address,undefined: a stand-alone program on the CPU, exit status 0"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "fir_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "pluto-gps-sim_amd", "csrc"), os.path.join(ROOT, "tools", "fir_asan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr):
        pytest.skip("%s cannot link the sanitizer runtimes" % cxx)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "clean" in run.stdout
