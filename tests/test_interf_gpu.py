"""Interference on the GPU (include/gpsbb.h gpsbb_interf_t, k_impair_iq, k_despread's INTERF instantiations): every host-bound
path that takes a set — the drop-in fill, the streaming ring, gpsbb_device_impair, the node driver in every layout, the
despreader's view and gpsbb-sim — bit for bit against apply_impair / view_host and pack_iq (the numpy restatement) of the plain
render of the same stream.  The clip counter must be numpy's count; every refusal leaves handle, stream, node and batch working
and the noise-only calls giving the bytes they gave."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_check as dc  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1


def emitters(pkg, delt):
    """a tone; a full-band chirp of 1024 samples; a pulsed chirp whose sweep (301) and gate (260 / 78, offset 17) divide nothing;
    a pulsed tone at -fs/2 with a gate of 77"""
    fs = 1.0 / delt
    e1 = pkg.interf_make(pkg.INTERF_CW, -6.0, 1000.0, delt=delt)
    e1.phase0 = 0xFEDCBA9876543210
    e2 = pkg.interf_make(pkg.INTERF_CHIRP, 3.0, -fs / 2, fs / 2, 1024 * delt, delt=delt)
    e3 = pkg.interf_make(pkg.INTERF_CHIRP, 0.0, -0.2 * fs, 0.27 * fs, 301 * delt, 260 * delt, 0.3, delt=delt)
    e3.pulse_offset, e3.phase0 = 17, 12345678901234567
    e4 = pkg.interf_make(pkg.INTERF_CW, 10.0, -fs / 2, pulse_period_s=77 * delt, duty=0.5, delt=delt)
    assert (e2.sweep, e3.sweep, e3.pulse_period, e3.pulse_on, e4.pulse_period) == (1024, 301, 260, 78, 77)
    return [e1, e2, e3, e4]


def impaired(pkg, iq, nz, st, fmt):
    """what a path with noise nz (or None), set st and format fmt must deliver for the plain int16 blocks iq, and the clips"""
    w, n = pkg.apply_impair(iq, nz, st)
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
def test_fill_with_interference_every_format(pkg, synth, oracle, fs, nsamp, nch, seed):
    """with noise, without noise, with an empty set; pageable and registered iq_out; end states and hazard counts are the plain
    call's; a NULL set is gpsbb_fill_block_noise"""
    L = pkg.lib()
    delt = 1.0 / fs
    ch = pkg.synth_descriptors(1, nch=nch, seed=seed)[0]
    want, _, _ = oracle.fill_blocks(ch, delt, nsamp)
    synth.hazards(reset=True)
    iq16, st16 = synth.fill_block(ch, delt, nsamp)
    hz16 = synth.hazards(reset=True)
    assert (iq16 == want[0]).all()
    s0 = 12345 + nsamp
    nz = pkg.Noise(7, s0, pkg.noise_sigma(45.0, 1.0, delt), 1, 0)
    full, empty = pkg.InterfSet(emitters(pkg, delt), 1, s0), pkg.InterfSet([], 1, s0)
    reg = np.zeros(nsamp * 4 + 4096, np.uint8)
    assert L.gpsbb_host_register(synth._h, reg.ctypes.data, reg.nbytes) == 0
    try:
        for fmt in FORMATS(pkg):
            nb = pkg.out_bytes(fmt, nsamp)
            for noise, st in ((nz, full), (None, full), (nz, empty), (None, empty)):
                exp, n = impaired(pkg, iq16, noise, st, fmt)
                if st is empty and noise is not None:   # the bytes of the noise call
                    assert (exp == pkg.pack_iq(pkg.apply_noise(iq16, 7, s0, nz.sigma, 1)[0], fmt)).all()
                for where in ("pageable", "registered+8"):
                    c0 = nclipped(pkg, synth)
                    if where == "pageable":
                        got, st_end = synth.fill_block(ch, delt, nsamp, fmt=fmt, noise=noise, interf=st)
                    else:
                        reg[:] = 0x5A
                        out = reg[8:8 + nb] if fmt else reg[8:8 + nb].view(np.int16).reshape(nsamp, 2)
                        got, st_end = synth.fill_block(ch, delt, nsamp, fmt=fmt, noise=noise, interf=st, out=out)
                        assert got.ctypes.data == reg.ctypes.data + 8
                        assert (reg[:8] == 0x5A).all() and (reg[8 + nb:] == 0x5A).all()
                    assert (got == exp).all(), (hex(fmt), where, noise is not None, st.n)
                    assert st_end.tobytes() == st16.tobytes()
                    assert synth.hazards(reset=True) == hz16
                    assert nclipped(pkg, synth) - c0 == n
            # NULL set: gpsbb_fill_block_noise
            buf = np.zeros(nb, np.uint8)
            assert L.gpsbb_fill_block_impair(synth._h, ch.ctypes.data, nch, delt, nsamp, fmt, C.byref(nz), None, buf.ctypes.data, None) == 0
            assert (buf == np.ascontiguousarray(impaired(pkg, iq16, nz, empty, fmt)[0]).view(np.uint8).ravel()).all()
    finally:
        assert L.gpsbb_host_unregister(synth._h, reg.ctypes.data) == 0


@pytest.mark.parametrize("nsamp", [4, 5, 8196, 8197])
def test_fill_with_impairments_small_shapes(pkg, synth, nsamp):
    """the shapes the blocks above never have.  4 samples: one 16-byte unit and no tail; 5: a ragged tail of two components for SC16
    and SC8; 8196: 2049 units, so the second chunk of 2048 holds a single one (the chunk loop, the guard per load, SC1's partial
    store); 8197: that and the tail.  Each at an odd and an even position — an SC1 block above always starts on an odd one, so
    its units never took the two-pair path — with the full set and noise, the set alone, an empty set with noise and the noise
    alone through the NULL-set call, in every format nsamp allows, pageable and 8 bytes into a registered buffer whose start is
    64-byte aligned: SC16's destination is then off its 16 bytes and takes the per-component path."""
    L = pkg.lib()
    fs, nch = 2.6e6, 12
    delt = 1.0 / fs
    ch = pkg.synth_descriptors(1, nch=nch, seed=106)[0]
    iq16, _ = synth.fill_block(ch, delt, nsamp)
    raw = np.zeros(nsamp * 4 + 4096 + 64, np.uint8)
    reg = raw[(-raw.ctypes.data) % 64:][:nsamp * 4 + 4096]
    assert reg.ctypes.data % 64 == 0
    assert L.gpsbb_host_register(synth._h, reg.ctypes.data, reg.nbytes) == 0
    try:
        for s0 in (12345, 12346):
            nz = pkg.Noise(7, s0, pkg.noise_sigma(45.0, 1.0, delt), 1, 0)
            full, empty = pkg.InterfSet(emitters(pkg, delt), 1, s0), pkg.InterfSet([], 1, s0)
            for fmt in FORMATS(pkg):
                if fmt == pkg.OUT_SC1 and nsamp % 4:
                    continue
                nb = pkg.out_bytes(fmt, nsamp)
                for noise, st in ((nz, full), (None, full), (nz, empty), (nz, None)):
                    exp, n = impaired(pkg, iq16, noise, empty if st is None else st, fmt)
                    exp = np.ascontiguousarray(exp).view(np.uint8).ravel()
                    assert exp.size == nb
                    for where in ("pageable", "registered+8"):
                        reg[:] = 0x5A
                        out = np.full(nb, 0x5A, np.uint8) if where == "pageable" else reg[8:8 + nb]
                        c0 = nclipped(pkg, synth)
                        assert L.gpsbb_fill_block_impair(synth._h, ch.ctypes.data, nch, delt, nsamp, fmt, C.byref(noise) if noise else None,
                                                         C.byref(st) if st is not None else None, out.ctypes.data, None) == 0
                        assert (out == exp).all(), (s0, hex(fmt), where, noise is not None, None if st is None else st.n)
                        assert nclipped(pkg, synth) - c0 == n
                        if where != "pageable":
                            assert (reg[:8] == 0x5A).all() and (reg[8 + nb:] == 0x5A).all()
    finally:
        assert L.gpsbb_host_unregister(synth._h, reg.ctypes.data) == 0


def test_interference_clip_counter(pkg, synth):
    """a tone of level 72 (crests of +-36 700) on 16 channels saturates at both ends: the counter is numpy's count, and SC8's own
    counts where it always did"""
    fs, nsamp = 25e6, 200000
    delt = 1.0 / fs
    ch = pkg.synth_descriptors(1, nch=16, seed=104)[0]
    iq16, _ = synth.fill_block(ch, delt, nsamp)
    big = pkg.interf_make(pkg.INTERF_CW, 20 * math.log10(72.0), 2.5e5, delt=delt)
    st = pkg.InterfSet([big], 0, 1)
    for noise in (None, pkg.Noise(3, 1, 3000.0, 0, 0)):
        for fmt in (pkg.OUT_SC16, pkg.OUT_SC8(7)):
            exp, n = impaired(pkg, iq16, noise, st, fmt)
            assert n > 1000
            c0, s0 = nclipped(pkg, synth), synth.info(pkg.INFO_SC8_CLIPPED)
            got, _ = synth.fill_block(ch, delt, nsamp, fmt=fmt, noise=noise, interf=st)
            assert (got == exp).all()
            assert nclipped(pkg, synth) - c0 == n
            if fmt != pkg.OUT_SC16:
                q = pkg.apply_impair(iq16, noise, st)[0].astype(np.int32) >> 7
                assert synth.info(pkg.INFO_SC8_CLIPPED) - s0 == int(((q < -128) | (q > 127)).sum())


# ---- the streaming ring -------------------------------------------------------------------------------------------------

def ring(pkg, synth, ch, fs, nsamp, bps, fmt, noise=None, interf=None, depth=8, plan=None):
    s = synth.stream(ch.shape[1], 1.0 / fs, nsamp, bps, depth=depth, flags=pkg.CHAIN_CARRIER, fmt=fmt, noise=noise, interf=interf)
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


def test_stream_with_interference_every_format(pkg, synth):
    fs, nsamp, bps, npush = 25e6, 100000, 2, 6
    delt = 1.0 / fs
    ch = pkg.synth_descriptors(bps * npush, nch=16, seed=105)
    s, iq16, st16, dg16 = ring(pkg, synth, ch, fs, nsamp, bps, pkg.OUT_SC16)
    s.close()
    assert (dg16 == pkg.block_digest_host(iq16)).all()
    em = emitters(pkg, delt)
    nz, js = pkg.Noise(11, 3, 6000.0, 0, 0), pkg.InterfSet(em, 0, 3)
    nz2, js2 = pkg.Noise(12, 1 << 40, 2000.0, 2, 0), pkg.InterfSet(em[1:3], 2, 1 << 40)
    half = npush // 2 * bps
    for fmt in FORMATS(pkg):
        c0 = nclipped(pkg, synth)
        s, got, st, dg = ring(pkg, synth, ch, fs, nsamp, bps, fmt, noise=nz, interf=js)
        exp, n = impaired(pkg, iq16, nz, js, fmt)
        assert (got == exp).all(), hex(fmt)
        assert st.tobytes() == st16.tobytes() and (dg == dg16).all()   # the render is the plain one
        assert nclipped(pkg, synth) - c0 == n
        # the rule, at the later call: a set elsewhere or with another shift is refused while nz is on, and nothing changes
        for bad in (pkg.InterfSet(em, 0, 4), pkg.InterfSet(em, 1, 3)):
            assert pkg.lib().gpsbb_stream_set_interf(s._s, C.byref(bad)) == BADARG
        assert pkg.lib().gpsbb_stream_set_noise(s._s, C.byref(nz2)) == BADARG
        # both moved: interference off, the noise to nz2, the set after it; slot 0 again as a new chain
        s.set_interf(None)
        s.set_noise(nz2)
        s.set_interf(js2)
        s.push(ch[:bps], new_chain=True)
        a, _ = s.pop()
        exp0, _ = impaired(pkg, iq16[:bps], nz2, js2, fmt)
        assert (a == exp0).all(), hex(fmt)
        # reset: back to the last sample0
        s.reset()
        s.push(ch[:bps])
        b, _ = s.pop()
        assert (b == exp0).all(), hex(fmt)
        # noise off: the set alone, from where the stream stands (one push on)
        s.set_noise(None)
        s.push(ch[bps:2 * bps])
        c, _ = s.pop()
        assert (c == impaired(pkg, iq16[bps:2 * bps], None, pkg.InterfSet(em[1:3], 2, (1 << 40) + bps * nsamp), fmt)[0]).all()
        # interference off too: the plain packing again
        s.set_interf(None)
        s.reset()
        s.push(ch[:bps])
        d, _ = s.pop()
        assert (d == pkg.pack_iq(iq16[:bps], fmt)).all()
        s.close()
        # set_interf in the middle of a stream without noise: the pushes before have none, the later ones start at its position
        s, got, _, dg = ring(pkg, synth, ch, fs, nsamp, bps, fmt, plan={npush // 2: lambda st: st.set_interf(js2)})
        s.close()
        e2, _ = impaired(pkg, iq16[half:], None, js2, fmt)
        assert (got == np.concatenate([pkg.pack_iq(iq16[:half], fmt), e2])).all(), hex(fmt)
        assert (dg == dg16).all()


# ---- gpsbb_device_impair ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nblocks,nsamp,sample0", [(1, 1, 0), (3, 1001, 5), (2, 70001, 2 ** 33 + 1), (1, 262144, 8)])
def test_device_impair_in_and_out_of_place(pkg, synth, nblocks, nsamp, sample0):
    """every launch but the first spans many sweeps (301, 1024) and gate periods (77, 260); sample0 odd and above 2^33"""
    import torch
    rng = np.random.default_rng(nsamp)
    iq = rng.integers(-20000, 20000, size=(nblocks, nsamp, 2)).astype(np.int16)
    ends = np.array([32767, -32768, 32767, -32768], np.int16)
    iq.reshape(-1)[:min(4, iq.size)] = ends[:min(4, iq.size)]
    em = emitters(pkg, 1.0 / 2.6e6)
    em[3].level_q16 = 30 << 16     # the pulsed tone at level 30: it saturates
    for noise in (pkg.Noise(0xFEEDFACECAFEBEEF, sample0, 9000.0, 0, 0), None):
        st = pkg.InterfSet(em, 0, sample0)
        exp, n = pkg.apply_impair(iq, noise, st)
        d = on_device(iq)
        o = torch.empty_like(d)
        c0 = nclipped(pkg, synth)
        synth.device_impair(d.data_ptr(), nblocks, nsamp, noise, st, d_dst=o.data_ptr())
        assert (o.cpu().numpy() == exp).all()
        assert (d.cpu().numpy() == iq).all()                   # the source is left alone
        assert nclipped(pkg, synth) - c0 == n
        synth.device_impair(d.data_ptr(), nblocks, nsamp, noise, st)   # in place
        assert (d.cpu().numpy() == exp).all()
    # NULL set: gpsbb_device_noise
    noise = pkg.Noise(5, sample0, 2000.0, 1, 0)
    d = on_device(iq)
    synth.device_impair(d.data_ptr(), nblocks, nsamp, noise, None)
    assert (d.cpu().numpy() == pkg.apply_noise(iq, 5, sample0, 2000.0, 1)[0]).all()


def test_device_impair_unaligned(pkg, synth):
    """source and destination 2 and 6 bytes into their buffers: the per-component path, the same bytes"""
    import torch
    nsamp = 40001
    rng = np.random.default_rng(9)
    iq = rng.integers(-3000, 3000, size=(1, nsamp, 2)).astype(np.int16)
    nz, st = pkg.Noise(5, 77, 1500.0, 3, 0), pkg.InterfSet(emitters(pkg, 1.0 / 2.6e6), 3, 77)
    for noise in (nz, None):
        d = on_device(np.concatenate([np.zeros(1, np.int16), iq.ravel(), np.zeros(1, np.int16)]))
        o = torch.full((2 * nsamp + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
        exp, _ = pkg.apply_impair(iq, noise, st)
        synth.device_impair(d.data_ptr() + 2, 1, nsamp, noise, st, d_dst=o.data_ptr() + 6)
        got = o.cpu().numpy()
        assert (got[3:3 + 2 * nsamp] == exp.ravel()).all()
        assert (got[:3] == 0x5A5A).all() and (got[3 + 2 * nsamp:] == 0x5A5A).all()
        synth.device_impair(d.data_ptr() + 2, 1, nsamp, noise, st)     # in place, unaligned
        dd = d.cpu().numpy()
        assert (dd[1:1 + 2 * nsamp] == exp.ravel()).all() and dd[0] == 0 and dd[-1] == 0


# ---- the node driver ----------------------------------------------------------------------------------------------------

def node_collect(pkg, ch, fs, nsamp, nshards, flags, fmt, noise, interf, feed=False):
    out = {}

    def sink(ptr, first, nb, shard):
        out[first] = pkg.iq_view(ptr, nb, nsamp, fmt).copy()
    with pkg.Node(nshards, ch.shape[1], 1.0 / fs, nsamp, 2, depth=2, flags=flags, devices=[0] * nshards, fmt=fmt,
                  noise=noise, interf=interf) as node:
        if feed:
            node.begin(sink)
            node.feed(ch[:5])
            node.feed(ch[5:])
            node.end()
        else:
            node.run(ch, sink)
    return np.concatenate([out[k] for k in sorted(out)])[:ch.shape[0]]


@pytest.mark.parametrize("layout", ["contiguous", "interleaved", "indexed", "feed"])
def test_node_interference_any_split(pkg, layout):
    fs, nsamp = 25e6, 100000
    ch = pkg.synth_descriptors(11, nch=16, seed=106)
    flags = {"contiguous": 0, "interleaved": pkg.NODE_INTERLEAVED, "indexed": pkg.NODE_INDEXED | pkg.NODE_CONCURRENT, "feed": 0}[layout]
    iq16 = node_collect(pkg, ch, fs, nsamp, 1, 0, pkg.OUT_SC16, None, None)
    nz, js = pkg.Noise(21, 999, 5000.0, 1, 0), pkg.InterfSet(emitters(pkg, 1.0 / fs), 1, 999)
    cases = [(pkg.OUT_SC16, nz), (pkg.OUT_SC8(4), nz), (pkg.OUT_SC1, None)] if layout == "contiguous" else [(pkg.OUT_SC8(4), nz), (pkg.OUT_SC16, None)]
    for fmt, noise in cases:
        exp, _ = impaired(pkg, iq16, noise, js, fmt)
        for nshards in (1, 3):
            got = node_collect(pkg, ch, fs, nsamp, nshards, flags, fmt, noise, js, feed=layout == "feed")
            assert (got == exp).all(), (layout, nshards, hex(fmt), noise is not None)


# ---- refusals -------------------------------------------------------------------------------------------------------------

def bad_sets(pkg, delt, s0, shift):
    def make(change):
        st = pkg.InterfSet(emitters(pkg, delt), shift, s0)
        change(st)
        return st

    def field(k, name, v):
        return lambda st: setattr(st.e[k], name, v)
    return [make(lambda st: setattr(st, "n", 5)), make(lambda st: setattr(st, "n", -1)), make(lambda st: setattr(st, "shift", 8)),
            make(lambda st: setattr(st, "shift", -1)), make(field(0, "kind", 2)), make(field(0, "level_q16", 0)),
            make(field(0, "level_q16", (1 << 27) + 1)), make(field(0, "sweep", 2)), make(field(1, "sweep", 1)),
            make(field(2, "pulse_on", 0)), make(field(2, "pulse_on", 261)), make(field(2, "pulse_offset", 260)),
            make(lambda st: setattr(st, "sample0", (1 << 63) - 5))]   # the range reaches 2^63


def test_refusals_leave_everything_usable(pkg, synth, oracle):
    L = pkg.lib()
    fs, nsamp, nch = 2.6e6, 30000, 12
    delt = 1.0 / fs
    ch = pkg.synth_descriptors(4, nch=nch, seed=107)
    iq16, _ = synth.fill_block(ch[0], delt, nsamp)
    good_nz = pkg.Noise(1, 0, 3000.0, 0, 0)
    good = pkg.InterfSet(emitters(pkg, delt), 0, 0)
    s = synth.stream(nch, delt, nsamp, 2, depth=2, flags=pkg.CHAIN_CARRIER, noise=good_nz, interf=good)
    b = synth.batch(ch[:1], delt, nsamp, flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    sums = b.despread(noise=good_nz, interf=good)
    buf = np.zeros(nsamp * 4, np.uint8)
    out = np.zeros(sums.shape, np.int64)
    d = on_device(iq16)
    dp = C.c_void_p(d.data_ptr())
    c0 = nclipped(pkg, synth)
    bad = bad_sets(pkg, delt, 0, 0)
    for k, st in enumerate(bad):
        for noise in (None, C.byref(good_nz)) if k < len(bad) - 1 else (None,):
            assert L.gpsbb_fill_block_impair(synth._h, ch[0].ctypes.data, nch, delt, nsamp, 0, noise, C.byref(st), buf.ctypes.data, None) == BADARG, k
            assert L.gpsbb_device_impair(synth._h, dp, dp, 1, nsamp, noise, C.byref(st)) == BADARG, k
            assert L.gpsbb_batch_despread_impaired(b._b, None, 0, noise, C.byref(st), 1, out.ctypes.data) == BADARG, k
        assert L.gpsbb_stream_set_interf(s._s, C.byref(st)) == BADARG, k
    # the rule: sample0 or shift unequal between the noise and the set
    for st in (pkg.InterfSet(emitters(pkg, delt), 0, 1), pkg.InterfSet(emitters(pkg, delt), 1, 0)):
        assert L.gpsbb_fill_block_impair(synth._h, ch[0].ctypes.data, nch, delt, nsamp, 0, C.byref(good_nz), C.byref(st), buf.ctypes.data, None) == BADARG
        assert L.gpsbb_device_impair(synth._h, dp, dp, 1, nsamp, C.byref(good_nz), C.byref(st)) == BADARG
        assert L.gpsbb_batch_despread_impaired(b._b, None, 0, C.byref(good_nz), C.byref(st), 1, out.ctypes.data) == BADARG
        assert L.gpsbb_stream_set_interf(s._s, C.byref(st)) == BADARG
    # a bad noise beside a good set; neither given
    worse = pkg.Noise(1, 0, float("nan"), 0, 0)
    assert L.gpsbb_device_impair(synth._h, dp, dp, 1, nsamp, C.byref(worse), C.byref(good)) == BADARG
    assert L.gpsbb_device_impair(synth._h, dp, dp, 1, nsamp, None, None) == BADARG
    # a ring in HBM takes no interference
    dev = synth.stream(nch, delt, nsamp, 2, depth=2, flags=pkg.CHAIN_CARRIER | pkg.STREAM_DEVICE_ONLY)
    assert L.gpsbb_stream_set_interf(dev._s, C.byref(good)) == BADARG and L.gpsbb_stream_set_interf(dev._s, None) == BADARG
    dev.close()
    assert (d.cpu().numpy() == iq16).all() and nclipped(pkg, synth) == c0    # nothing ran
    # ... and everything goes on with what it had: the impaired calls, and the noise-only calls with the bytes they gave
    exp, _ = pkg.apply_impair(iq16, good_nz, good)
    got, _ = synth.fill_block(ch[0], delt, nsamp, noise=good_nz, interf=good)
    assert (got == exp).all()
    s.push(ch[:2])
    a, _ = s.pop()
    assert (a[0] == exp).all()
    s.close()
    assert (b.despread(noise=good_nz, interf=good) == sums).all()
    rep = dc.replicas(oracle, ch[:1], delt, nsamp, chain=True)
    assert (sums == pkg.despread_host(pkg.view_host(iq16[None], pkg.OUT_SC16, good_nz, interf=good), rep, 1)).all()
    assert (b.despread(noise=good_nz) == pkg.despread_host(pkg.view_host(iq16[None], pkg.OUT_SC16, good_nz), rep, 1)).all()
    b.close()
    expn, _ = pkg.apply_noise(iq16, 1, 0, 3000.0, 0)
    assert (synth.fill_block(ch[0], delt, nsamp, noise=good_nz)[0] == expn).all()
    synth.device_noise(d.data_ptr(), 1, nsamp, good_nz)
    assert (d.cpu().numpy() == expn).all()
    # the node: none with rings in HBM; bad sets and the rule refused; run_digest refused while a set is on
    with pkg.Node(1, nch, delt, nsamp, 2, devices=[0], flags=pkg.NODE_DEVICE_ONLY) as node:
        with pytest.raises(pkg.GpsbbError) as e:
            node.set_interf(good)
        assert e.value.rc == BADARG
    with pkg.Node(1, nch, delt, nsamp, 2, devices=[0]) as node:
        for st in bad[:-1]:
            with pytest.raises(pkg.GpsbbError) as e:
                node.set_interf(st)
            assert e.value.rc == BADARG
        node.set_noise(good_nz)
        for st in (pkg.InterfSet(emitters(pkg, delt), 0, 1), pkg.InterfSet(emitters(pkg, delt), 1, 0)):
            with pytest.raises(pkg.GpsbbError):
                node.set_interf(st)
        got = np.zeros((4, nsamp, 2), np.int16)

        def sink(ptr, first, nb, shard):
            got[first:first + nb] = pkg.iq_view(ptr, nb, nsamp)
        node.run(ch, sink)
        assert (got[0] == expn).all()       # the refused sets left the node with its noise alone
        node.set_interf(good)
        with pytest.raises(pkg.GpsbbError) as e:
            node.set_noise(pkg.Noise(1, 5, 3000.0, 0, 0))
        assert e.value.rc == BADARG
        node.run(ch, sink)
        assert (got[0] == exp).all()
        node.set_noise(None)
        with pytest.raises(pkg.GpsbbError) as e:
            node.run_digest(ch)
        assert e.value.rc == BADARG
        node.set_interf(None)
        node.run_digest(ch)


# ---- the despreader's view ----------------------------------------------------------------------------------------------

_cases = {}


def geometry(pkg, oracle, name):
    if name not in _cases:
        g = [g for g in dc.geometries(pkg) if g["name"] == name][0]
        delt = 1.0 / g["fs"]
        iq, _, _ = oracle.fill_blocks(g["ch"], delt, g["nsamp"], chain=True)
        _cases[name] = dict(g, delt=delt, iq=iq, rep=dc.replicas(oracle, g["ch"], delt, g["nsamp"], chain=True))
    return _cases[name]


@pytest.mark.parametrize("name,shift", [("pd wide", 0), ("ev", 1)])
def test_despread_impaired_every_view(pkg, synth, oracle, name, shift):
    """a state per tile (2.6 MS/s) and per two tiles (25 MS/s, behind the lap pre-pass): SC16, SC8 and SC1, with and without noise,
    against despread_host(view_host(..., interf=)); on a buffer gpsbb_device_impair filled the plain despread gives the same
    sums; the existing call gives what it gave"""
    import torch
    g = geometry(pkg, oracle, name)
    nb = g["ch"].shape[0]
    s0 = (1 << 33) + 4321
    nz = pkg.Noise(0xBEEF, s0, pkg.noise_sigma(45.0, 1.0, g["delt"]), shift, 0)
    js = pkg.InterfSet(emitters(pkg, g["delt"]), shift, s0)
    b = synth.batch(g["ch"], g["delt"], g["nsamp"], flags=pkg.CHAIN_CARRIER)
    b.run()
    synth.sync()
    assert synth.info(pkg.INFO_LAST_VARIANT) == g["variant"]
    ext = torch.zeros(nb * g["nsamp"] * 2, dtype=torch.int16, device="cuda")
    synth.device_impair(b.device_iq(), nb, g["nsamp"], nz, js, d_dst=ext.data_ptr())
    bad = []
    for view in (pkg.OUT_SC16, pkg.OUT_SC8(5), pkg.OUT_SC1):
        for noise in (nz, None):
            want = pkg.despread_host(pkg.view_host(g["iq"], view, noise, interf=js), g["rep"], 3)
            if not (b.despread(view=view, noise=noise, seg_tiles=3, interf=js) == want).all():
                bad.append("view 0x%x noise %s: differs from view_host" % (view, noise is not None))
            if noise is not None and not (b.despread(view=view, seg_tiles=3, d_iq=ext.data_ptr()) == want).all():
                bad.append("view 0x%x: the external impaired buffer gives other sums" % view)
        if not (b.despread(view=view, noise=nz, seg_tiles=3) == pkg.despread_host(pkg.view_host(g["iq"], view, nz), g["rep"], 3)).all():
            bad.append("view 0x%x: the noise-only despread changed" % view)
        empty = pkg.InterfSet([], shift, s0)
        if not (b.despread(view=view, noise=nz, seg_tiles=3, interf=empty) == b.despread(view=view, noise=nz, seg_tiles=3)).all():
            bad.append("view 0x%x: an empty set is not the noise call" % view)
    b.close()
    del ext
    assert not bad, "\n".join(bad)


# ---- gpsbb-sim ------------------------------------------------------------------------------------------------------------

def sim(pkg, out, *args):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    r = subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100", "-s", "2600000",
                        *args, "-o", out], check=True, stderr=subprocess.PIPE, text=True, timeout=600)
    return r.stderr


def test_gpsbb_sim_interference_same_file_on_every_path(pkg, tmp_path):
    pkg.build_frontend()
    nsamp, delt = 300000, 1.0 / 2.6e6
    plain = str(tmp_path / "plain.bin")
    sim(pkg, plain, "-d", "0.3", "-b", "16")
    iq16 = np.fromfile(plain, np.int16).reshape(-1, nsamp, 2)
    jargs = ["-J", "cw,-6,1000", "-J", "chirp,3,-1.3e6,1.3e6,0.001,0.01,0.5"]
    em = [pkg.interf_make(pkg.INTERF_CW, -6, 1000, delt=delt),
          pkg.interf_make(pkg.INTERF_CHIRP, 3, -1.3e6, 1.3e6, 0.001, 0.01, 0.5, delt=delt)]
    assert (em[1].sweep, em[1].pulse_period, em[1].pulse_on) == (2600, 26000, 13000)
    nz, js = pkg.Noise(7, 0, pkg.noise_sigma(45.0, 1.0, delt), 1, 0), pkg.InterfSet(em, 1, 0)
    for bits, fmt in (("16", pkg.OUT_SC16), ("8", pkg.OUT_SC8(5)), ("1", pkg.OUT_SC1)):
        exp, n = impaired(pkg, iq16, nz, js, fmt)
        paths = (["-d", "0.3"], ["-d", "0.3", "-F"], ["-d", "0.3", "-G", "2", "-g", "0,0"])
        if bits == "16":
            paths += (["-d", "0.3", "-R"], ["-d", "0.3", "-G", "2", "-g", "0,0", "-C"])
        for path in paths:
            f = str(tmp_path / ("b%s%s.bin" % (bits, "".join(path))))
            err = sim(pkg, f, *path, "-b", bits, "-W", "45,1", "-w", "7", *jargs)
            got = np.fromfile(f, exp.dtype).reshape(exp.shape)
            assert (got == exp).all(), (bits, path)
            if "-G" not in path and "-F" not in path:
                assert int(err.split("noise components clipped: ")[1].split()[0]) == n
    # without -W: the shift from -j; -k keeps the bytes of the full file
    expj, _ = impaired(pkg, iq16, None, pkg.InterfSet(em, 2, 0), pkg.OUT_SC16)
    for path in (["-d", "0.3"], ["-d", "0.3", "-F"]):
        f = str(tmp_path / ("j%s.bin" % "".join(path)))
        sim(pkg, f, *path, "-j", "2", *jargs)
        assert (np.fromfile(f, np.int16).reshape(-1, nsamp, 2) == expj).all(), path
    f = str(tmp_path / "k1.bin")
    sim(pkg, f, "-d", "0.3", "-j", "2", "-k", "1", *jargs)
    assert (np.fromfile(f, np.int16).reshape(-1, nsamp, 2) == expj[1:2]).all()
