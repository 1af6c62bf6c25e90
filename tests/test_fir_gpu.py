"""gpsbb_device_fir on the GPU (k_fir): every comparison is == on every output sample, the history handed on and the clip count
against fir_host fed with view_host's output (tools/fir_check.py), on the smallest shapes at which the kernel can go wrong — odd
decimations and even lengths, output counts around one tile and a ragged third, a buffer shorter than the history, the
accumulators at the end of their range, the negative halves of the rounding, every impairment, a call split in four — every
refusal; and end to end: six satellites rendered at 10.4 MS/s, filtered and decimated to 2.6 MS/s, then acquired and tracked by
the existing chain unchanged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fir_check as fc  # noqa: E402
import track_check as tc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1


def clips(pkg, synth):
    return synth.info(pkg.INFO_SC8_CLIPPED), synth.info(pkg.INFO_NOISE_CLIPPED)


@pytest.mark.parametrize("T,D", fc.SHAPES)
def test_1_lane_and_tile_map(pkg, synth, T, D):
    """Random full-range int16 IQ with +-32767 and -32768 in it, random taps of both signs with the sum of |h| at 65535; output counts
    1, 2, FIR_TILE - 1, FIR_TILE, FIR_TILE + 1 and 2 FIR_TILE + 3; hist_in NULL and random."""
    assert pkg.FIR_TILE == 256
    bad = []
    for M in fc.outputs(pkg):
        iq = fc.ac.random_iq(max(M * D, 5), 0xF100 + T)[:M * D]
        fir = fc.random_fir(pkg, T, D, 15, T * 31 + D)
        bad += fc.check(pkg, synth, iq, fir, None, what="M %d" % M)
        bad += fc.check(pkg, synth, iq, fir, fc.random_hist(T, 0xF1), what="M %d with history" % M)
    big = fc.ac.random_iq(64, 0xF100 + T)
    assert {32767, -32767, -32768} <= set(big[:, 0].tolist()) and {32767, -32768} <= set(big[:, 1].tolist())
    assert not bad, "\n".join(bad)


def test_2_ends(pkg, synth):
    """Five spare samples of 0x7fff behind d_iq and a canary behind d_out (fir_check.on_device): neither is read into a sum nor
    written.  nsamp = D: one output.  nsamp < T - 1: hist_out mixes hist_in and w."""
    fir = fc.random_fir(pkg, 33, 4, 15, 0xE1)
    iq = fc.ac.random_iq(4 * 300, 0xE2)
    iq5 = np.concatenate([iq, np.full((5, 2), 0x7FFF, np.int16)])
    hist = fc.random_hist(33, 0xE3)
    want = fc.mirror(pkg, iq, fir, hist)
    bad = fc.compare(fc.on_device(pkg, synth, iq5, fir, hist, spare=5), want, "5 spare samples")
    one = fc.on_device(pkg, synth, iq[:4], fir, hist)
    bad += fc.compare(one, fc.mirror(pkg, iq[:4], fir, hist), "nsamp = D")
    assert one[0].shape == (1, 2) and (one[1][:28] == hist[4:]).all() and (one[1][28:] == iq[:4]).all()
    short = fc.on_device(pkg, synth, iq[:20], fir, hist)
    bad += fc.compare(short, fc.mirror(pkg, iq[:20], fir, hist), "nsamp < T - 1")
    assert (short[1][:12] == hist[20:]).all() and (short[1][12:] == iq[:20]).all()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shift", [0, 16])
def test_3_accumulator_range(pkg, synth, shift):
    """Every component -32768 under h = {32767, 32767, 1}: acc = -65535 * 32768, the end of the range.  == the mirror and the closed
    form; shift 0 clips every component."""
    M = pkg.FIR_TILE + 5
    iq = np.full((M, 2), -32768, np.int16)
    fir = pkg.Fir([32767, 32767, 1], 1, shift)
    hist = np.full((2, 2), -32768, np.int16)
    got = fc.on_device(pkg, synth, iq, fir, hist)
    bad = fc.compare(got, fc.mirror(pkg, iq, fir, hist))
    assert not bad, "\n".join(bad)
    acc = -65535 * 32768
    want = max((acc + (1 << 15)) >> 16, -32768) if shift else -32768
    assert (got[0] == want).all() and got[2] == (0 if shift else 2 * M) and want == (-32767 if shift else -32768)


def test_4_rounding_and_identity(pkg, synth):
    """h = {1} with shift 0 and h = {16384} with shift 14 return the buffer; h = {1, 1} with shift 1 on sums of -1, -3, 1, 3, -2:
    halves go toward +infinity."""
    iq = fc.ac.random_iq(pkg.FIR_TILE + 9, 0xD1)
    for fir in (pkg.Fir([1], 1, 0), pkg.Fir([16384], 1, 14), pkg.fir_make(1, 1)):
        y, hist, clipped = fc.on_device(pkg, synth, iq, fir)
        assert (y == iq).all() and hist.shape == (0, 2) and clipped == 0
    v = np.array([[0, -1], [-1, -2], [0, 1], [1, 2], [-3, 1], [1, -32768], [-32768, 32767]], np.int16)
    fir = pkg.Fir([1, 1], 1, 1)
    got = fc.on_device(pkg, synth, v, fir)
    assert not fc.compare(got, fc.mirror(pkg, v, fir))
    assert got[0][:, 0].tolist() == [0, 0, 0, 1, -1, -1, -16383] and got[0][:, 1].tolist() == [0, -1, 0, 2, 2, -16383, 0]


@pytest.mark.parametrize("impair", ["plain", "noise", "noise+chirp", "chirp"])
def test_5_views(pkg, synth, impair):
    """(33, 4) plain, with a gpsbb_noise_t whose sample0 lies above 2^32, with noise and a chirp, with the chirp alone.  The handle's
    clip counters do not move; the impaired result differs from the plain one."""
    iq = fc.ac.random_iq(4 * (pkg.FIR_TILE + 40), 0xC1)
    iq = (iq.astype(np.int32) // 4).astype(np.int16)   # (room for the impairments: the view does not sit on its clamp)
    fir = pkg.fir_make(33, 4)
    nz = pkg._as_noise(fc.NOISE) if "noise" in impair else None
    js = fc.chirp_set(pkg) if "chirp" in impair else None
    assert fc.NOISE["sample0"] > 1 << 32
    before = clips(pkg, synth)
    got = fc.on_device(pkg, synth, iq, fir, None, nz, js)
    bad = fc.compare(got, fc.mirror(pkg, iq, fir, None, nz, js), impair)
    assert not bad, "\n".join(bad)
    assert clips(pkg, synth) == before
    if impair != "plain":
        assert (got[0] != fc.mirror(pkg, iq, fir)[0]).any()


def test_6_resume(pkg, synth):
    """With noise on: one call == calls of D, FIR_TILE * D - D, a piece shorter than T - 1, and the rest, the histories handed on."""
    T, D = 33, 4
    fir = pkg.fir_make(T, D)
    n = D * (2 * pkg.FIR_TILE + 50)
    iq = (fc.ac.random_iq(n, 0xB1).astype(np.int32) // 4).astype(np.int16)
    whole = fc.on_device(pkg, synth, iq, fir, None, fc.NOISE)
    bad = fc.compare(whole, fc.mirror(pkg, iq, fir, None, fc.NOISE), "whole")
    parts, hist, nclip, at = [], None, 0, 0
    for k in (D, pkg.FIR_TILE * D - D, 5 * D, None):
        k = n - at if k is None else k
        nz, _ = fc.advanced(pkg, fc.NOISE, None, at)
        y, hist, c = fc.on_device(pkg, synth, iq[at:at + k], fir, hist, nz)
        parts.append(y)
        nclip += c
        at += k
    assert at == n and 5 * D < T - 1
    bad += fc.compare((np.concatenate(parts), hist, nclip), whole, "split")
    assert not bad, "\n".join(bad)


def test_7_refusals(pkg, synth, oracle):
    """Every GPSBB_E_BADARG of the definition and the served neighbour of each; after every refusal the handle still renders a block
    bit-exactly, and d_out, hist_out and clipped are as they were."""
    import torch
    L = pkg.lib()
    n = 4000
    t = torch.zeros((n + 8, 2), dtype=torch.int16, device="cuda")
    out = torch.full((n + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    good = pkg.fir_make(33, 4)
    ch = pkg.synth_descriptors(1, nch=4, seed=31)[0]
    delt = 1.0 / fc.FS
    want_iq = oracle.fill_blocks(ch[None, :], delt, 1500)[0][0]
    hout = np.full((128, 2), 0x77, np.int16)
    clipped = C.c_uint64(12345)

    def rc(fir=good, src=t.data_ptr(), dst=out.data_ptr(), nsamp=n, nz=None, js=None, null_fir=False, h=None):
        r = L.gpsbb_device_fir(synth._h if h is None else h, C.c_void_p(src) if src else None, nsamp, None if nz is None else C.byref(nz),
                               None if js is None else C.byref(js), None if null_fir else C.byref(fir), None, hout.ctypes.data,
                               C.c_void_p(dst) if dst else None, C.byref(clipped))
        if r != 0:
            torch.cuda.synchronize()
            assert (hout == 0x77).all() and clipped.value == 12345 and bool((out == 0x5A5A).all())
        return r

    def still_renders():
        iq, _ = synth.fill_block(ch, delt, 1500)
        assert (iq == want_iq).all()

    def served(**kw):
        r = rc(**kw)
        hout[:] = 0x77
        clipped.value = 12345
        out.fill_(0x5A5A)
        torch.cuda.synchronize()
        return r == 0

    def with_(**f):
        c = pkg.Fir.from_buffer_copy(good)
        for k, v in f.items():
            setattr(c, k, v)
        return c

    def taps(h, D=1, shift=0):
        return pkg.Fir(h, D, shift)

    assert served()
    still_renders()
    nz_ok = pkg.Noise(1, 5, 100.0, 1, 0)
    cw = pkg.interf_make(pkg.INTERF_CW, 0.0, 1000.0, delt=delt)
    js5 = pkg.InterfSet([cw], 0, 0)
    js5.n = 5
    cases = [("d_iq NULL", dict(src=0)), ("fir NULL", dict(null_fir=True)), ("d_out NULL", dict(dst=0)), ("d_iq misaligned", dict(src=t.data_ptr() + 2)),
             ("d_out misaligned", dict(dst=out.data_ptr() + 2)), ("nsamp 0", dict(nsamp=0)), ("nsamp < 0", dict(nsamp=-4)),
             ("nsamp no multiple of D", dict(nsamp=n - 1)), ("T 0", dict(fir=with_(ntaps=0))), ("T beyond", dict(fir=with_(ntaps=pkg.FIR_MAX_TAPS + 1))),
             ("D 0", dict(fir=with_(decim=0))), ("D 17", dict(fir=with_(decim=17))), ("shift -1", dict(fir=with_(shift=-1))),
             ("shift 17", dict(fir=with_(shift=17))), ("sum |h| 65536", dict(fir=taps([32767, -32767, 2]))),
             ("d_out inside d_iq", dict(dst=t.data_ptr() + 4 * (n - 1))), ("d_iq inside d_out", dict(src=out.data_ptr() + 4 * (n // 4 - 1))),
             ("d_out == d_iq", dict(dst=t.data_ptr())),
             ("noise sigma 0", dict(nz=pkg.Noise(1, 0, 0.0, 0, 0))), ("noise shift 8", dict(nz=pkg.Noise(1, 0, 100.0, 8, 0))),
             ("a set of 5 emitters", dict(js=js5)), ("a set's shift 8", dict(js=pkg.InterfSet([cw], 8, 0))),
             ("noise and set apart in sample0", dict(nz=nz_ok, js=pkg.InterfSet([cw], 1, 6))),
             ("noise and set apart in shift", dict(nz=nz_ok, js=pkg.InterfSet([cw], 2, 5)))]
    for what, kw in cases:
        assert rc(**kw) == BADARG, what
        still_renders()
    assert rc(h=0) == BADARG
    # the neighbours of the refusals are served
    assert served(nsamp=4) and served(fir=with_(ntaps=1)) and served(fir=taps([0] * pkg.FIR_MAX_TAPS)) and served(fir=with_(decim=1))
    assert served(fir=with_(decim=16)) and served(fir=with_(shift=0)) and served(fir=with_(shift=16)) and served(fir=taps([32767, -32767, 1]))
    # (the ranges touch: [t, t + n / 2) into what follows it; [out + n / 8, out + n / 8 + n / 2) into [out, out + n / 8))
    assert served(dst=t.data_ptr() + 4 * (n // 2), nsamp=n // 2) and served(src=out.data_ptr() + 4 * (n // 8), nsamp=n // 2)
    assert served(nz=nz_ok, js=pkg.InterfSet([cw], 1, 5)) and served(nz=nz_ok) and served(js=pkg.InterfSet([cw], 1, 5))
    still_renders()


def sim(pkg, out, fs, *args):
    """gpsbb-sim in a fresh child process under its own time limit, 0.3 s of signal -> what it wrote to stderr"""
    import subprocess
    from conftest import GOLDEN
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    r = subprocess.run(["timeout", "-k", "10", "120", exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100", "-s", str(fs),
                        "-d", "0.3", *args, "-o", out], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def test_9_the_tool(pkg, tmp_path):
    """gpsbb-sim -D: -D 1,1 writes the bytes of the same command without -D; -s 2600000 -D 4,33 writes fir_host of the file that
    -s 10400000 writes without -D (blocks of the same 0.1154 s: -n 1200000 there, 300000 here); the same with -b 8 and -W 45,1:
    noise at the rendered rate, against the mirror."""
    pkg.build_frontend()
    plain, same = str(tmp_path / "plain.bin"), str(tmp_path / "d1.bin")
    sim(pkg, plain, 2600000)
    sim(pkg, same, 2600000, "-D", "1,1")
    with open(plain, "rb") as f, open(same, "rb") as g:
        a, b = f.read(), g.read()
    assert len(a) == 3 * 300000 * 4 and a == b
    wide, dec, dec8 = str(tmp_path / "wide.bin"), str(tmp_path / "dec.bin"), str(tmp_path / "dec8.bin")
    sim(pkg, wide, 10400000, "-n", "1200000")
    err = sim(pkg, dec, 2600000, "-D", "4,33")
    iq = np.fromfile(wide, np.int16).reshape(-1, 2)
    assert iq.shape[0] == 3 * 1200000
    fir = pkg.fir_make(33, 4)
    want, _, clipped = pkg.fir_host(pkg.view_host(iq), fir)
    got = np.fromfile(dec, np.int16).reshape(-1, 2)
    assert got.shape == want.shape and (got == want).all()
    assert int(err.split("components clipped: ")[1].split()[0]) == clipped
    sim(pkg, dec8, 2600000, "-D", "4,33", "-b", "8", "-W", "45,1")
    nz = pkg.Noise(1, 0, pkg.noise_sigma(45.0, 1.0, 1.0 / 10.4e6), 1, 0)
    want8, _, _ = pkg.fir_host(pkg.view_host(iq, pkg.OUT_SC16, nz), fir)
    exp = pkg.pack_iq(want8.reshape(3, 300000, 2), pkg.OUT_SC8(5))
    got8 = np.fromfile(dec8, exp.dtype).reshape(exp.shape)
    assert (got8 == exp).all()


def test_10_the_tool_refuses(pkg, tmp_path):
    """-D together with -A, -P, -k, -G, -S or -R, and a -D that is not well formed: one line each, exit status 1, before a GPU is touched"""
    import subprocess
    from conftest import GOLDEN
    pkg.build_frontend()
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    for extra in (["-A", "100"], ["-P", "1000"], ["-k", "1"], ["-G", "2"], ["-S", str(tmp_path / "s.json")], ["-R"]):
        r = subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-D", "4", *extra, "-o", str(tmp_path / "x.bin")],
                           stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and r.stderr.count("ERROR: -D not together with") == 1, (extra, r.stderr)
    for arg in ("0", "17", "4,0", "4,130", "4,33,1.5", "4,33,0.8,200", "4,33,0.8,60,1", "x", "4;33"):
        r = subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-D", arg, "-o", str(tmp_path / "x.bin")],
                           stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and "ERROR: -D wants" in r.stderr, (arg, r.stderr)


def test_8_end_to_end(pkg, synth):
    """tools/acq_check.e2e_descriptors (six satellites) rendered at 10.4 MS/s as one block of 5 200 000 samples, device_fir with
    fir_make(33, 4) into 1 300 000 samples at 2.6 MS/s: == the mirror of the read-back render, nothing clipped.  Then the existing
    chain unchanged at 2.6 MS/s: per PRN the carrier within 1 Hz, one histogram bin at the descriptor's edge, 16 or 17 bits equal up
    to sign.  The six first code wraps lie more than the filter's delay before lag 2600: no epoch numbering moves."""
    import torch
    ch = tc.e2e_descriptors(pkg)
    lags = fc.e2e_first_wraps(pkg, ch)
    print("first wraps at output lags %s" % ["%.1f" % v for v in lags])
    assert all(0 <= v and v + 4 < 2600 for v in lags)
    fir = fc.e2e_fir(pkg)
    acq, trk = tc.e2e_acq_cfg(pkg, pkg.OUT_SC16), tc.e2e_trk_cfg(pkg)
    out = torch.zeros((tc.E2E_NSAMP, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    b = synth.batch(ch, 1.0 / fc.FS_IN, fc.E2E_NSAMP_IN)
    try:
        b.run()
        synth.sync()
        hist, clipped = synth.device_fir(b.device_iq(), fc.E2E_NSAMP_IN, fir, out.data_ptr())
        rows = synth.device_acquire(out.data_ptr(), tc.E2E_ACQ_NSAMP, acq)
        st = tc.e2e_seeds(pkg, rows, acq)
        _, recs = synth.device_track(out.data_ptr(), tc.E2E_NSAMP, trk, st)
        iq, _ = b.read()
    finally:
        b.close()
    want = pkg.fir_host(pkg.view_host(iq[0]), fir)
    bad = fc.compare((out.cpu().numpy(), hist, clipped), want, "the decimated stream")
    assert clipped == 0
    more, (min_pi, max_pq) = tc.e2e_findings(pkg, ch, recs)
    print("min |P.i| %.3g, max |P.q| %.3g after epoch %d; records %s" % (min_pi, max_pq, tc.E2E_SKIP, [r.size for r in recs]))
    assert not bad + more, "\n".join(bad + more)
