"""Interference excision without a GPU: csrc/gpsbb_exc.h's plain-C definition against the numpy mirror excise_host, the identity
an empty plan must be, an independent float64 numpy.fft overlap-add, an int64 shadow of every inverse stage (nothing nears 2^31),
the clamp, the split rule with both counters, gpsbb_exc_make's window, gpsbb_exc_from_psd on a spectrum with one hot bin, every
refusal of the two host functions, the end-to-end figures on the mirrors, and tools/exc_asan.cpp built and run under the host
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
import exc_check as ec  # noqa: E402
from exc_check import ac  # noqa: E402

BADARG = -1


def gaussian(n, sigma, seed):
    return np.clip(np.rint(np.random.default_rng(seed).standard_normal((n, 2)) * sigma), -32768, 32767).astype(np.int16)


def identity_inputs(N, nblk=6):
    n = nblk * (N // 2)
    return {"full-scale random": ac.random_iq(n, 0xE600 + N), "Gaussian sigma 100": gaussian(n, 100, 0xE601 + N), "Gaussian sigma 5": gaussian(n, 5, 0xE602 + N)}


@pytest.mark.parametrize("log2n", [6, 7, 12])
def test_1_plain_c_is_the_mirror(pkg, log2n):
    """exc_host of csrc/gpsbb_exc.h == excise_host: random legal windows with 0 and 16384 in them, random masks, thr zero and at the
    median cell power, hist NULL and given, 1 and 5 blocks"""
    N, H = 1 << log2n, 1 << (log2n - 1)
    iq = ac.random_iq(5 * H, 0xE610 + log2n)
    hist = ac.random_iq(N, 0xE611 + log2n)
    e = ec.lane_map_plan(pkg, log2n, iq)
    w = e.window()
    assert 0 in w.tolist() and 16384 in w.tolist() and e.thr > 0 and 0 < e.bins().sum() < N
    for plan in (e, e.copy(thr=0), e.copy(bins=())):
        for h in (None, hist):
            for n in (H, 5 * H):
                want = pkg.excise_host(iq[:n], plan, h)
                got = pkg.excise_plain_c(iq[:n], plan, h)
                bad = ec.compare(got[:4], want, "N %d thr %d hist %s nsamp %d" % (N, plan.thr, h is not None, n))
                assert not bad, "\n".join(bad)
    assert pkg.excise_host(iq, e)[3] > pkg.excise_host(iq, e.copy(thr=0))[3] > 0


@pytest.mark.parametrize("log2n", ec.LOG2NS)
def test_2_identity(pkg, log2n):
    """an empty plan (gpsbb_exc_make's) gives the input delayed by H: exactly for log2n <= 10, within 1 LSB at 11 and 12 (the
    figures of the definition's prototype), on full-scale random and on Gaussian samples of sigma 100 and sigma 5; nothing is
    clipped or excised"""
    N, H = 1 << log2n, 1 << (log2n - 1)
    e = pkg.exc_make(log2n)
    for name, w in identity_inputs(N).items():
        out, hist, clipped, excised = pkg.excise_host(w, e)
        d = int(np.abs(out[H:].astype(np.int64) - w[:-H].astype(np.int64)).max())
        print("N %d %s: largest difference %d" % (N, name, d))
        assert d <= (0 if log2n <= 10 else 1), name
        assert (clipped, excised) == (0, 0) and (hist == w[-N:]).all() and np.abs(out[:H].astype(np.int64)).max() <= (0 if log2n <= 10 else 1)


def float_ola(w, exc, cells):
    """windowed overlap-add in float64 with numpy.fft: the same window, the same zeroed cells, no rounding anywhere"""
    L = int(exc.log2n)
    N, H = 1 << L, 1 << (L - 1)
    nblk = w.shape[0] // H
    x = np.concatenate([np.zeros(N), w[:, 0].astype(np.float64) + 1j * w[:, 1]])
    seg = x[np.arange(nblk + 1)[:, None] * H + np.arange(N)[None, :]] * (exc.window().astype(np.float64) / 16384.0)[None, :]
    X = np.fft.fft(seg, axis=1)
    X[cells] = 0
    y = np.fft.ifft(X, axis=1)
    o = (y[:-1, H:] + y[1:, :H]).reshape(nblk * H)
    return np.stack([o.real, o.imag], 1)


# the largest |excise_host - float_ola| measured over test_3's inputs, per log2n; the test asserts twice as much
FLOAT_MEASURED = {6: 0.5022, 9: 0.5694, 12: 1.0340}


@pytest.mark.parametrize("log2n", [6, 9, 12])
def test_3_against_float_fft(pkg, log2n):
    """against an independent float64 numpy.fft windowed overlap-add under the same window with the mirror's own zeroed cells:
    the lane map's plan (about 10 % of the bins masked, thr at the median cell power) on full-scale random and on Gaussian samples
    of sigma 100 and 5.  The bound is twice the largest difference measured on these inputs"""
    N = 1 << log2n
    worst = 0.0
    for name, w in identity_inputs(N).items():
        e = ec.lane_map_plan(pkg, log2n, w)
        cells = []
        out, _, clipped, excised = pkg.excise_host(w, e, cells=cells)
        ref = np.clip(float_ola(w, e, np.concatenate(cells)), -32768, 32767)
        d = float(np.abs(out - ref).max())
        print("N %d %s: largest difference %.4f LSB, %d cells zeroed, %d clipped" % (N, name, d, excised, clipped))
        assert excised > 0
        worst = max(worst, d)
    assert worst <= 2 * FLOAT_MEASURED[log2n]


@pytest.mark.parametrize("log2n", [6, 9, 12])
def test_4_no_wrap(pkg, log2n):
    """an int64 shadow of the mirror keeps every inverse intermediate far below 2^31 for a constant -32768, alternating full
    scale, full-scale tones on and between bins, +-full-scale random and an impulse, each under masks of 0, 1/6, 1/2 and 5/6 of
    the bins; the plain-C definition, in int32, reports the same peak: it never wrapped"""
    N = 1 << log2n
    worst = 0
    for name, w in ec.stress_inputs(N).items():
        for plan in ec.stress_plans(pkg, log2n):
            shadow = []
            want = pkg.excise_host(w, plan, shadow=shadow)
            got = pkg.excise_plain_c(w, plan)
            assert not ec.compare(got[:4], want, name)
            assert max(shadow) == got[4] < 1 << 31, name
            worst = max(worst, max(shadow))
    print("N %d: the largest inverse intermediate 2^%.2f" % (N, np.log2(max(worst, 1))))
    assert worst < 2 ** 28.5 + 64


def test_5_clamp(pkg):
    """a full-scale square wave of period N / 4 with every bin masked but 4 and N - 4: the fundamental alone reaches 4 / pi of full
    scale, so the clamp works"""
    for log2n in (6, 9):
        w, plan = ec.square_case(pkg, log2n)
        out, _, clipped, excised = pkg.excise_host(w, plan)
        print("N %d: clipped %d, excised %d" % (1 << log2n, clipped, excised))
        assert clipped > 0 and excised == 4 * ((1 << log2n) - 2)
        assert out.max() == 32767 and out.min() == -32768
        assert not ec.compare(pkg.excise_plain_c(w, plan)[:4], (out, _, clipped, excised))


def test_6_split(pkg):
    """one call == any split of it at multiples of H with the history handed on: out concatenated, clipped and excised added"""
    log2n, N, H = 7, 128, 64
    sq, sq_plan = ec.square_case(pkg, log2n)                 # (the clamp works in this one)
    rnd = ac.random_iq(13 * H, 0xE620)
    h0 = ac.random_iq(N, 0xE622)
    for iq, e in ((rnd, ec.lane_map_plan(pkg, log2n, rnd)), (np.concatenate([rnd[:5 * H], sq, sq]), sq_plan)):
        whole = pkg.excise_host(iq, e, h0)
        assert whole[3] > 0 and (whole[2] > 0 or e.thr > 0)
        for cuts in ((H,), (3 * H,), (2 * H, 3 * H, 12 * H)):
            outs, hist, clipped, excised, at = [], h0, 0, 0, 0
            for c in cuts + (iq.shape[0],):
                o, hist, cl, ex = pkg.excise_host(iq[at:c], e, hist)
                outs.append(o)
                clipped, excised, at = clipped + cl, excised + ex, c
            assert not ec.compare((np.concatenate(outs), hist, clipped, excised), whole, "cuts %r" % (cuts,))


def test_7_exc_make(pkg):
    """gpsbb_exc_make: the periodic Hann window, legal, an empty mask, no threshold; its refusals leave e as it was"""
    L = pkg.lib()
    for log2n in ec.LOG2NS:
        N, H = 1 << log2n, 1 << (log2n - 1)
        e = pkg.exc_make(log2n)
        w = e.window()
        assert (e.log2n, e.thr) == (log2n, 0) and not e.bins().any() and not bytes(e.mask).strip(b"\0") and pkg.exc_ok(e)
        assert w[0] == 0 and w[H] == 16384 and (w[:H] + w[H:] == 16384).all() and w.min() >= 0 and w.max() <= 16384
        assert (w[:H] == np.rint(16384 * 0.5 * (1 - np.cos(2 * np.pi * np.arange(H) / N)))).all()
        assert not np.frombuffer(e.win, np.int16)[N:].any()
    e = pkg.Exc(6, 5, [7] * 64, [True] * 3)
    keep = bytes(e)
    assert L.gpsbb_exc_make(C.byref(e), 5) == BADARG and L.gpsbb_exc_make(C.byref(e), 13) == BADARG and bytes(e) == keep
    assert L.gpsbb_exc_make(None, 6) == BADARG
    assert C.sizeof(pkg.Exc) == 8720
    assert all(pkg.exp_lib().gpsbb_test_exc_run(n) == pkg.exc_run(n) for n in range(6, 13)) and pkg.exp_lib().gpsbb_test_exc_run(13) == -1


def test_8_exc_from_psd(pkg):
    """a flat spectrum with one hot bin: the mask holds that bin alone, thr is floor(10^(thr_db / 10) * med * 4^shift / nseg)"""
    for log2n in (6, 10):
        N = 1 << log2n
        p = pkg.Psd(log2n, N // 2, 2, [1] * N)
        psd = np.full(N, 1000, np.uint64)
        psd[2::2] = 1001                      # N / 2 entries of 1000, N / 2 - 1 of 1001 and the hot one: the lower median is 1000
        psd[N - 3] = 1000 * 100
        e = pkg.exc_from_psd(pkg.exc_make(log2n), psd, p, 8, 10.0, 6.0)
        assert np.flatnonzero(e.bins()).tolist() == [N - 3]
        assert e.thr == int(np.floor(10.0 ** 0.6 * 1000 * 16 / 8)) and (e.window() == pkg.exc_make(log2n).window()).all()
        e2 = pkg.exc_from_psd(e, psd, p, 8, 0.0, 0.0)
        assert not e2.bins().any() and e2.thr == 0
        e3 = pkg.exc_from_psd(e, psd, p, 8, 25.0, -1.0)     # 20 dB above the median is not 25
        assert not e3.bins().any() and e3.thr == 0
        e4 = pkg.exc_from_psd(e, psd, p, 8, 19.9, 0.0)
        assert e4.bins().sum() == 1


def test_9_refusals_of_the_host_functions(pkg):
    """every GPSBB_E_BADARG of gpsbb_exc_from_psd leaves e as it was; the neighbours are served"""
    L = pkg.lib()
    N = 64
    p = pkg.Psd(6, 32, 0, [1] * N)
    psd = np.full(N, 1 << 40, np.uint64)
    e = pkg.exc_make(6).copy(thr=77, bins=[True, False, True])
    keep = bytes(e)

    def rc(e_=e, psd_=psd, p_=p, nseg=4, mask_db=3.0, thr_db=3.0):
        return L.gpsbb_exc_from_psd(None if e_ is None else C.byref(e_), None if psd_ is None else psd_.ctypes.data, None if p_ is None else C.byref(p_),
                                    nseg, mask_db, thr_db)

    cases = [("e NULL", dict(e_=None)), ("psd NULL", dict(psd_=None)), ("p NULL", dict(p_=None)), ("another log2n", dict(p_=p.copy(log2n=7))),
             ("nseg 0", dict(nseg=0)), ("nseg beyond", dict(nseg=(1 << 20) + 1)), ("shift -1", dict(p_=p.copy(shift=-1))), ("shift 31", dict(p_=p.copy(shift=31))),
             ("mask_db nan", dict(mask_db=float("nan"))), ("mask_db inf", dict(mask_db=float("inf"))), ("thr_db nan", dict(thr_db=float("nan"))),
             ("thr_db -inf", dict(thr_db=float("-inf"))), ("thr does not fit", dict(p_=p.copy(shift=12), nseg=1, thr_db=3.0)),
             ("e's log2n 5", dict(e_=e.copy(log2n=5), p_=p.copy(log2n=5))), ("e's log2n 13", dict(e_=e.copy(log2n=13), p_=p.copy(log2n=13)))]
    for what, kw in cases:
        assert rc(**kw) == BADARG and bytes(e) == keep, what
    assert rc(p_=p.copy(shift=11), nseg=1, thr_db=3.0) == 0 and e.thr == int(np.floor(10.0 ** 0.3 * 2.0 ** 40 * 4.0 ** 11))
    assert rc(nseg=1 << 20) == 0 and rc(p_=p.copy(shift=30), nseg=1 << 20, thr_db=0.0) == 0 and e.thr == 0 and not e.bins().any()
    for bad_plan in (e.copy(log2n=5), e.copy(log2n=13)):
        with pytest.raises(ValueError):
            pkg.excise_host(np.zeros((64, 2), np.int16), bad_plan)
    w = e.window()
    for n, v in ((0, -1), (3, int(w[3]) + 1), (40, int(w[40]) - 1)):
        w2 = w.copy()
        w2[n] = v
        with pytest.raises(ValueError):
            pkg.excise_host(np.zeros((64, 2), np.int16), pkg.Exc(6, 0, w2))
        with pytest.raises(pkg.GpsbbError):
            pkg.excise_plain_c(np.zeros((64, 2), np.int16), pkg.Exc(6, 0, w2))
    for n in (0, 31, 33, 48):
        with pytest.raises(ValueError):
            pkg.excise_host(np.zeros((n, 2), np.int16), e)
        with pytest.raises(pkg.GpsbbError):
            pkg.excise_plain_c(np.zeros((n, 2), np.int16), e)
    pkg.excise_host(np.zeros((32, 2), np.int16), e)
    w3 = np.concatenate([np.full(32, 16384), np.zeros(32)]).astype(np.int16)          # the ends of the range are legal
    assert pkg.excise_plain_c(np.zeros((32, 2), np.int16), pkg.Exc(6, 0, w3))[2:4] == (0, 0)


def test_e2e_figures_on_the_mirror(pkg):
    """the end-to-end cases of the GPU test on the CPU oracle's render: the search is defeated by the CW emitter and by the chirp
    and whole again after excision, before any GPU is asked"""
    bad = ec.e2e_cpu(pkg)
    assert not bad, "\n".join(bad)


def test_exc_asan(tmp_path):
    """tools/exc_asan.cpp under -fsanitize=address,undefined: a stand-alone program on the CPU, exit status 0"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "exc_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "pluto-gps-sim_amd", "csrc"), os.path.join(ROOT, "tools", "exc_asan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr):
        pytest.skip("%s cannot link the sanitizer runtimes" % cxx)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "clean" in run.stdout
