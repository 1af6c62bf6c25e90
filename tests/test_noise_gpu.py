"""Receiver noise on the GPU (include/gpsbb.h gpsbb_noise_t, k_impair_iq<FMT, true, false>): every host-bound path that takes noise — the drop-in fill
(pageable and registered), the streaming ring, gpsbb_device_noise, the node driver in every layout and gpsbb-sim — bit for bit
against apply_noise and pack_iq (the numpy restatement) of the noiseless render of the same stream.  The clip counter must be
numpy's count; every refusal leaves the handle, stream and node working."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BADARG = -1


@pytest.fixture(scope="module")
def table(pkg):
    return pkg.noise_table()


def noisy(pkg, iq, nz, fmt, table):
    """what a path with noise nz and format fmt must deliver for the noiseless int16 blocks iq, and the noise clips"""
    w, n = pkg.apply_noise(iq, nz["seed"], nz["sample0"], nz["sigma"], nz["shift"], table)
    return pkg.pack_iq(w, fmt), n


def nclipped(pkg, synth):
    return synth.info(pkg.INFO_NOISE_CLIPPED)


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


FORMATS = lambda pkg: (pkg.OUT_SC16, pkg.OUT_SC8(5), pkg.OUT_SC1)  # noqa: E731


# ---- the drop-in fill --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,nsamp,nch,seed", [(2.6e6, 300000, 12, 101), (15.8565e6, 158564, 16, 102), (25e6, 250000, 16, 103)])
def test_fill_with_noise_every_format(pkg, synth, oracle, table, fs, nsamp, nch, seed):
    """pageable and registered iq_out; the end states are the plain call's; a NULL noise is gpsbb_fill_block_ex"""
    L = pkg.lib()
    ch = pkg.synth_descriptors(1, nch=nch, seed=seed)[0]
    want, _, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
    iq16, st16 = synth.fill_block(ch, 1.0 / fs, nsamp)
    assert (iq16 == want[0]).all()
    nz = {"seed": 7, "sample0": 12345 + nsamp, "sigma": pkg.noise_sigma(45.0, 1.0, 1.0 / fs), "shift": 1}
    reg = np.zeros(nsamp * 4 + 4096, np.uint8)
    assert L.gpsbb_host_register(synth._h, reg.ctypes.data, reg.nbytes) == 0
    try:
        for fmt in FORMATS(pkg):
            exp, n = noisy(pkg, iq16, nz, fmt, table)
            nb = pkg.out_bytes(fmt, nsamp)
            for where in ("pageable", "registered", "registered+8"):
                c0 = nclipped(pkg, synth)
                if where == "pageable":
                    got, st = synth.fill_block(ch, 1.0 / fs, nsamp, fmt=fmt, noise=nz)
                else:
                    at = 8 if where == "registered+8" else 0
                    reg[:] = 0x5A
                    out = reg[at:at + nb] if fmt else reg[at:at + nb].view(np.int16).reshape(nsamp, 2)
                    got, st = synth.fill_block(ch, 1.0 / fs, nsamp, fmt=fmt, noise=nz, out=out)
                    assert got.ctypes.data == reg.ctypes.data + at
                    assert (reg[:at] == 0x5A).all() and (reg[at + nb:] == 0x5A).all()
                assert (got == exp).all(), (hex(fmt), where)
                assert st.tobytes() == st16.tobytes()
                assert nclipped(pkg, synth) - c0 == n
            # NULL noise: the bytes of gpsbb_fill_block_ex
            buf = np.zeros(nb, np.uint8)
            assert L.gpsbb_fill_block_noise(synth._h, ch.ctypes.data, nch, 1.0 / fs, nsamp, fmt, None, buf.ctypes.data, None) == 0
            assert (buf == np.ascontiguousarray(pkg.pack_iq(iq16, fmt)).view(np.uint8).ravel()).all()
    finally:
        assert L.gpsbb_host_unregister(synth._h, reg.ctypes.data) == 0


def test_noise_clip_counter(pkg, synth, table):
    """sigma = 30 000 at shift 0 on 16 channels saturates thousands of components: the counter is numpy's count"""
    fs, nsamp = 25e6, 200000
    ch = pkg.synth_descriptors(1, nch=16, seed=104)[0]
    iq16, _ = synth.fill_block(ch, 1.0 / fs, nsamp)
    nz = {"seed": 3, "sample0": 1, "sigma": 30000.0, "shift": 0}
    for fmt in (pkg.OUT_SC16, pkg.OUT_SC8(7)):
        exp, n = noisy(pkg, iq16, nz, fmt, table)
        assert n > 1000
        c0, s0 = nclipped(pkg, synth), synth.info(pkg.INFO_SC8_CLIPPED)
        got, _ = synth.fill_block(ch, 1.0 / fs, nsamp, fmt=fmt, noise=nz)
        assert (got == exp).all()
        assert nclipped(pkg, synth) - c0 == n
        if fmt != pkg.OUT_SC16:     # SC8's own saturations of the noisy value are counted where they always were
            w, _ = pkg.apply_noise(iq16, 3, 1, 30000.0, 0, table)
            q = w.astype(np.int32) >> 7
            assert synth.info(pkg.INFO_SC8_CLIPPED) - s0 == int(((q < -128) | (q > 127)).sum())


# ---- the streaming ring -------------------------------------------------------------------------------------------------

def ring(pkg, synth, ch, fs, nsamp, bps, fmt, noise=None, depth=8, plan=None):
    """push every slot of ch (with digests), then pop them all; plan: {push index: callable(stream)} run before that push"""
    s = synth.stream(ch.shape[1], 1.0 / fs, nsamp, bps, depth=depth, flags=pkg.CHAIN_CARRIER, fmt=fmt, noise=noise)
    npush = ch.shape[0] // bps
    out, digs, sts = [], [], []
    for k in range(npush):
        if plan and k in plan:
            plan[k](s)
        s.push(ch[k * bps:(k + 1) * bps], digest=True)
    for k in range(npush):
        iq, st, dg = s.pop_digest()
        out.append(iq)
        sts.append(st)
        digs.append(dg)
    return s, np.concatenate(out), np.concatenate(sts), np.concatenate(digs)


def test_stream_with_noise_every_format(pkg, synth, table):
    fs, nsamp, bps, npush = 25e6, 100000, 2, 6
    ch = pkg.synth_descriptors(bps * npush, nch=16, seed=105)
    s, iq16, st16, dg16 = ring(pkg, synth, ch, fs, nsamp, bps, pkg.OUT_SC16)
    s.close()
    assert (dg16 == pkg.block_digest_host(iq16)).all()
    nz = {"seed": 11, "sample0": 3, "sigma": 6000.0, "shift": 0}
    nz2 = {"seed": 12, "sample0": 1 << 40, "sigma": 2000.0, "shift": 2}
    half = npush // 2 * bps
    for fmt in FORMATS(pkg):
        c0 = nclipped(pkg, synth)
        s, got, st, dg = ring(pkg, synth, ch, fs, nsamp, bps, fmt, noise=nz)
        exp, n = noisy(pkg, iq16, nz, fmt, table)
        assert (got == exp).all(), hex(fmt)
        assert st.tobytes() == st16.tobytes() and (dg == dg16).all()
        assert nclipped(pkg, synth) - c0 == n
        # a new PUSH_NEW_CHAIN stream at an explicit position: slot 0 again, at nz2
        s.set_noise(nz2)
        s.push(ch[:bps], new_chain=True)
        a, _ = s.pop()
        exp0, _ = noisy(pkg, iq16[:bps], nz2, fmt, table)
        assert (a == exp0).all(), hex(fmt)
        # reset: back to the last sample0
        s.reset()
        s.push(ch[:bps])
        b, _ = s.pop()
        assert (b == exp0).all(), hex(fmt)
        # noise off: the plain packing again
        s.set_noise(None)
        s.reset()
        s.push(ch[:bps])
        c, _ = s.pop()
        assert (c == pkg.pack_iq(iq16[:bps], fmt)).all()
        s.close()
        # set_noise in the middle: the pushes before keep theirs, the later ones start at nz2's position
        s, got, _, dg = ring(pkg, synth, ch, fs, nsamp, bps, fmt, noise=nz, plan={npush // 2: lambda st: st.set_noise(nz2)})
        s.close()
        e1, _ = noisy(pkg, iq16[:half], nz, fmt, table)
        e2, _ = noisy(pkg, iq16[half:], nz2, fmt, table)
        assert (got == np.concatenate([e1, e2])).all(), hex(fmt)
        assert (dg == dg16).all()


# ---- gpsbb_device_noise -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nblocks,nsamp,sample0", [(1, 1, 0), (3, 1001, 5), (2, 70001, 2 ** 33 + 1), (1, 262144, 8)])
def test_device_noise_in_and_out_of_place(pkg, synth, table, nblocks, nsamp, sample0):
    import torch
    rng = np.random.default_rng(nsamp)
    iq = rng.integers(-20000, 20000, size=(nblocks, nsamp, 2)).astype(np.int16)
    ends = np.array([32767, -32768, 32767, -32768], np.int16)
    iq.reshape(-1)[:min(4, iq.size)] = ends[:min(4, iq.size)]
    nz = {"seed": 0xFEEDFACECAFEBEEF, "sample0": sample0, "sigma": 30000.0, "shift": 0}
    exp, n = pkg.apply_noise(iq, nz["seed"], sample0, nz["sigma"], 0, table)
    d = on_device(iq)
    o = torch.empty_like(d)
    c0 = nclipped(pkg, synth)
    synth.device_noise(d.data_ptr(), nblocks, nsamp, nz, d_dst=o.data_ptr())
    assert (o.cpu().numpy() == exp).all()
    assert (d.cpu().numpy() == iq).all()                   # the source is left alone
    assert nclipped(pkg, synth) - c0 == n
    synth.device_noise(d.data_ptr(), nblocks, nsamp, nz)   # in place
    assert (d.cpu().numpy() == exp).all()


def test_device_noise_unaligned(pkg, synth, table):
    """source and destination 2 and 6 bytes into their buffers: the per-component path, the same bytes"""
    import torch
    nsamp = 40001
    rng = np.random.default_rng(9)
    iq = rng.integers(-3000, 3000, size=(1, nsamp, 2)).astype(np.int16)
    d = on_device(np.concatenate([np.zeros(1, np.int16), iq.ravel(), np.zeros(1, np.int16)]))
    o = torch.full((2 * nsamp + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    nz = {"seed": 5, "sample0": 77, "sigma": 1500.0, "shift": 3}
    exp, _ = pkg.apply_noise(iq, 5, 77, 1500.0, 3, table)
    synth.device_noise(d.data_ptr() + 2, 1, nsamp, nz, d_dst=o.data_ptr() + 6)
    got = o.cpu().numpy()
    assert (got[3:3 + 2 * nsamp] == exp.ravel()).all()
    assert (got[:3] == 0x5A5A).all() and (got[3 + 2 * nsamp:] == 0x5A5A).all()
    synth.device_noise(d.data_ptr() + 2, 1, nsamp, nz)     # in place, unaligned
    assert (d.cpu().numpy()[1:1 + 2 * nsamp] == exp.ravel()).all()


# ---- the node driver ----------------------------------------------------------------------------------------------------

def node_collect(pkg, ch, fs, nsamp, nshards, flags, fmt, noise, feed=False):
    out = {}

    def sink(ptr, first, nb, shard):
        out[first] = pkg.iq_view(ptr, nb, nsamp, fmt).copy()
    with pkg.Node(nshards, ch.shape[1], 1.0 / fs, nsamp, 2, depth=2, flags=flags, devices=[0] * nshards, fmt=fmt,
                  noise=noise) as node:
        if feed:
            node.begin(sink)
            node.feed(ch[:5])
            node.feed(ch[5:])
            node.end()
        else:
            node.run(ch, sink)
    return np.concatenate([out[k] for k in sorted(out)])[:ch.shape[0]]


@pytest.mark.parametrize("layout", ["contiguous", "interleaved", "indexed", "feed"])
def test_node_noise_any_split(pkg, table, layout):
    fs, nsamp = 25e6, 100000
    ch = pkg.synth_descriptors(11, nch=16, seed=106)
    flags = {"contiguous": 0, "interleaved": pkg.NODE_INTERLEAVED, "indexed": pkg.NODE_INDEXED | pkg.NODE_CONCURRENT, "feed": 0}[layout]
    iq16 = node_collect(pkg, ch, fs, nsamp, 1, 0, pkg.OUT_SC16, None)
    nz = {"seed": 21, "sample0": 999, "sigma": 5000.0, "shift": 1}
    for fmt in ((pkg.OUT_SC16, pkg.OUT_SC8(4), pkg.OUT_SC1) if layout == "contiguous" else (pkg.OUT_SC8(4),)):
        exp, _ = noisy(pkg, iq16, nz, fmt, table)
        for nshards in (1, 3):
            got = node_collect(pkg, ch, fs, nsamp, nshards, flags, fmt, nz, feed=layout == "feed")
            assert (got == exp).all(), (layout, nshards, hex(fmt))


# ---- refusals -------------------------------------------------------------------------------------------------------------

BAD = [{"sigma": float("nan"), "shift": 0}, {"sigma": 0.0, "shift": 0}, {"sigma": -1.0, "shift": 0},
       {"sigma": 2.0 ** 20 + 1, "shift": 0}, {"sigma": float("inf"), "shift": 0}, {"sigma": 100.0, "shift": 8},
       {"sigma": 100.0, "shift": -1}]


def test_refusals_leave_everything_usable(pkg, synth, table):
    L = pkg.lib()
    fs, nsamp, nch = 2.6e6, 30000, 12
    ch = pkg.synth_descriptors(4, nch=nch, seed=107)
    iq16, _ = synth.fill_block(ch[0], 1.0 / fs, nsamp)
    good = {"seed": 1, "sample0": 0, "sigma": 3000.0, "shift": 0}
    s = synth.stream(nch, 1.0 / fs, nsamp, 2, depth=2, flags=pkg.CHAIN_CARRIER, noise=good)
    buf = np.zeros(nsamp * 4, np.uint8)
    d = on_device(iq16)
    for b in BAD:
        nz = pkg._as_noise(dict(seed=1, sample0=0, **b))
        assert L.gpsbb_fill_block_noise(synth._h, ch[0].ctypes.data, nch, 1.0 / fs, nsamp, 0, C.byref(nz), buf.ctypes.data, None) == BADARG
        assert L.gpsbb_stream_set_noise(s._s, C.byref(nz)) == BADARG
        assert L.gpsbb_device_noise(synth._h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), 1, nsamp, C.byref(nz)) == BADARG
    assert L.gpsbb_device_noise(synth._h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), 1, nsamp, None) == BADARG
    # ... a ring in HBM takes no noise
    dev = synth.stream(nch, 1.0 / fs, nsamp, 2, depth=2, flags=pkg.CHAIN_CARRIER | pkg.STREAM_DEVICE_ONLY)
    assert L.gpsbb_stream_set_noise(dev._s, C.byref(pkg._as_noise(good))) == BADARG
    assert L.gpsbb_stream_set_noise(dev._s, None) == BADARG
    dev.close()
    # ... and everything goes on with the noise it had
    exp, _ = pkg.apply_noise(iq16, 1, 0, 3000.0, 0, table)
    got, _ = synth.fill_block(ch[0], 1.0 / fs, nsamp, noise=good)
    assert (got == exp).all()
    s.push(ch[:2])
    a, _ = s.pop()
    assert (a[0] == exp).all()
    s.close()
    synth.device_noise(d.data_ptr(), 1, nsamp, good)
    assert (d.cpu().numpy() == exp).all()
    # the node: no noise with rings in HBM; bad noise refused; run_digest refused while noise is set
    with pkg.Node(1, nch, 1.0 / fs, nsamp, 2, devices=[0], flags=pkg.NODE_DEVICE_ONLY) as node:
        with pytest.raises(pkg.GpsbbError) as e:
            node.set_noise(good)
        assert e.value.rc == BADARG
    with pkg.Node(1, nch, 1.0 / fs, nsamp, 2, devices=[0]) as node:
        for b in BAD:
            with pytest.raises(pkg.GpsbbError) as e:
                node.set_noise(dict(seed=1, sample0=0, **b))
            assert e.value.rc == BADARG
        node.set_noise(good)
        with pytest.raises(pkg.GpsbbError) as e:
            node.run_digest(ch)
        assert e.value.rc == BADARG
        got = np.zeros((4, nsamp, 2), np.int16)

        def sink(ptr, first, nb, shard):
            got[first:first + nb] = pkg.iq_view(ptr, nb, nsamp)
        node.run(ch, sink)
        assert (got[0] == exp).all()
        node.set_noise(None)
        node.run_digest(ch)


# ---- gpsbb-sim ------------------------------------------------------------------------------------------------------------

def sim(pkg, out, *args):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    r = subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100", "-s", "2600000",
                        *args, "-o", out], check=True, stderr=subprocess.PIPE, text=True, timeout=600)
    return r.stderr


def test_gpsbb_sim_noise_same_file_on_every_path(pkg, tmp_path, table):
    pkg.build_frontend()
    nsamp = 300000
    plain = str(tmp_path / "plain.bin")
    sim(pkg, plain, "-d", "0.3", "-b", "16")
    iq16 = np.fromfile(plain, np.int16).reshape(-1, nsamp, 2)
    nz = {"seed": 7, "sample0": 0, "sigma": pkg.noise_sigma(45.0, 1.0, 1.0 / 2.6e6), "shift": 1}
    for bits, fmt in (("16", pkg.OUT_SC16), ("8", pkg.OUT_SC8(5)), ("1", pkg.OUT_SC1)):
        exp, n = noisy(pkg, iq16, nz, fmt, table)
        files = []
        for path in (["-d", "0.3"], ["-d", "0.3", "-F"], ["-d", "0.3", "-G", "2", "-g", "0,0"]):
            f = str(tmp_path / ("b%s%s.bin" % (bits, "".join(path))))
            err = sim(pkg, f, *path, "-b", bits, "-W", "45,1", "-w", "7")
            got = np.fromfile(f, exp.dtype).reshape(exp.shape)
            assert (got == exp).all(), (bits, path)
            if "-G" not in path and "-F" not in path:
                assert int(err.split("noise components clipped: ")[1].split()[0]) == n
            files.append(open(f, "rb").read())
        assert files[0] == files[1] == files[2]
    # -k keeps the bytes of the full file
    f = str(tmp_path / "k1.bin")
    sim(pkg, f, "-d", "0.3", "-W", "45,1", "-w", "7", "-k", "1")
    exp, _ = noisy(pkg, iq16, nz, pkg.OUT_SC16, table)
    assert (np.fromfile(f, np.int16).reshape(-1, nsamp, 2) == exp[1:2]).all()
