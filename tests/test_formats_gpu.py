"""The smaller output formats on the GPU (include/gpsbb.h GPSBB_OUT_SC8 / GPSBB_OUT_SC1): the packing kernel on crafted int16, and
every host-bound path that takes a format — the drop-in fill (pageable and registered), the streaming ring, the node driver and
gpsbb-sim — against pack_iq (the numpy reference) of the same path's int16 output, which is itself checked against the golden
vectors or the CPU oracle.  The SC8 clip counter must be numpy's count, exactly."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BADARG = -1
V = [-32768, -17, -16, -1, 0, 1, 15, 16, 4095, 4096, 32767]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def clips(iq, shift):
    q = np.asarray(iq, np.int32) >> shift
    return int(((q < -128) | (q > 127)).sum())


def clipped(pkg, synth):
    return synth.info(pkg.INFO_SC8_CLIPPED)


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


def pinned(nbytes):
    import torch
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True).numpy()


def crafted(nblocks, nsamp, seed):
    """int16 blocks with every hand-worked value, every shift boundary 2^s - 1, 2^s, -2^s, -2^s - 1 and random fill"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-32768, 32768, size=nblocks * nsamp * 2).astype(np.int16)
    edges = list(V)
    for s in range(16):
        edges += [(1 << s) - 1, -(1 << s), -(1 << s) - 1, min((1 << s), 32767), 127 << s & 0x7fff, 128 << s & 0x7fff]
    edges = np.array(edges, np.int64).clip(-32768, 32767).astype(np.int16)
    k = min(a.size, edges.size)
    a[:k] = edges[:k]
    a[-k:] = edges[:k][::-1]
    return a.reshape(nblocks, nsamp, 2)


# ---- the packing kernel alone: gpsbb_device_pack ----------------------------------------------------------------------

@pytest.mark.parametrize("nblocks,nsamp", [(1, 1), (1, 3), (2, 5), (3, 1001), (1, 70001), (2, 262146), (1, 300000)])
def test_device_pack_sc8_every_shift(pkg, synth, nblocks, nsamp):
    """ragged nsamp (the n % 8 tail), a block that is several rounds of the kernel, pageable and pinned destinations"""
    iq = crafted(nblocks, nsamp, nsamp)
    d = on_device(iq)
    for shift in range(16):
        fmt = pkg.OUT_SC8(shift)
        c0 = clipped(pkg, synth)
        out = synth.device_pack(d.data_ptr(), nblocks, nsamp, fmt) if shift % 2 else \
            synth.device_pack(d.data_ptr(), nblocks, nsamp, fmt, out=pinned(nblocks * nsamp * 2))
        assert out.dtype == np.int8 and out.shape == (nblocks, nsamp, 2)
        assert (out == pkg.pack_iq(iq, fmt)).all(), shift
        assert clipped(pkg, synth) - c0 == clips(iq, shift), shift


@pytest.mark.parametrize("nblocks,nsamp", [(1, 4), (3, 4), (2, 12), (3, 4000), (5, 65540), (2, 300000)])
def test_device_pack_sc1_multi_block(pkg, synth, nblocks, nsamp):
    iq = crafted(nblocks, nsamp, 7 + nsamp)
    d = on_device(iq)
    c0 = clipped(pkg, synth)
    want = pkg.pack_iq(iq, pkg.OUT_SC1)
    got = synth.device_pack(d.data_ptr(), nblocks, nsamp, pkg.OUT_SC1)
    assert got.dtype == np.uint8 and got.shape == (nblocks, nsamp // 4)
    assert (got == want).all()
    got = synth.device_pack(d.data_ptr(), nblocks, nsamp, pkg.OUT_SC1, out=pinned(nblocks * nsamp // 4))
    assert (got == want).all()
    assert clipped(pkg, synth) == c0                      # SC1 clips nothing
    # SC16 through the same call is the plain copy
    assert (synth.device_pack(d.data_ptr(), nblocks, nsamp, pkg.OUT_SC16) == iq).all()


def test_device_pack_unaligned_source_and_destination(pkg, synth):
    """a block that starts 4 bytes into a buffer (nsamp odd) and a destination at an odd address: the per-byte path, same bytes"""
    iq = crafted(1, 40001, 3)
    d = on_device(np.concatenate([np.zeros((1, 1, 2), np.int16), iq], axis=1))
    src = d.data_ptr() + 4
    buf = np.zeros(2 * 40001 + 17, np.uint8)
    for fmt in (pkg.OUT_SC8(5), pkg.OUT_SC8(0)):
        c0 = clipped(pkg, synth)
        got = synth.device_pack(src, 1, 40001, fmt)
        assert (got == pkg.pack_iq(iq, fmt)).all()
        assert clipped(pkg, synth) - c0 == clips(iq, (fmt >> 12) & 15)
        buf[:] = 0xEE
        rc = pkg.lib().gpsbb_device_pack(synth._h, C.c_void_p(src), 1, 40001, fmt, C.c_void_p(buf.ctypes.data + 3))
        assert rc == 0
        assert (buf[3:3 + 2 * 40001].view(np.int8) == pkg.pack_iq(iq, fmt).ravel()).all()
        assert (buf[:3] == 0xEE).all() and (buf[3 + 2 * 40001:] == 0xEE).all()
    iq1 = crafted(1, 40000, 4)
    d1 = on_device(np.concatenate([np.zeros((1, 1, 2), np.int16), iq1], axis=1))
    assert (synth.device_pack(d1.data_ptr() + 4, 1, 40000, pkg.OUT_SC1) == pkg.pack_iq(iq1, pkg.OUT_SC1)).all()


# ---- the drop-in fill --------------------------------------------------------------------------------------------------

def test_fill_block_golden_static_F(pkg, synth):
    z = np.load(os.path.join(GOLDEN, "static_F.npz"))
    fs, nsamp = float(z["fs"]), int(z["nsamp"])
    desc = z["desc"].view(pkg.CHAN_DTYPE).reshape(z["desc"].shape[0], -1)
    want_st = z["end_state"].view(pkg.STATE_DTYPE).reshape(desc.shape)
    for k in range(desc.shape[0]):
        iq, st16 = synth.fill_block(desc[k], 1.0 / fs, nsamp)
        assert sha(iq) == str(z["iq_sha256"][k]), k
        for fmt in (pkg.OUT_SC8(4), pkg.OUT_SC8(5), pkg.OUT_SC1):
            c0 = clipped(pkg, synth)
            got, st = synth.fill_block(desc[k], 1.0 / fs, nsamp, fmt=fmt)
            assert (got == pkg.pack_iq(iq, fmt)).all(), (k, hex(fmt))
            assert st.tobytes() == st16.tobytes()
            assert clipped(pkg, synth) - c0 == (clips(iq, 4) if fmt == pkg.OUT_SC8(4) else 0)
            if k == 0 and fmt == pkg.OUT_SC8(5):
                assert (want_st[k]["carr_phase"] == st["carr_phase"]).all()


@pytest.mark.parametrize("fs,nsamp,nch,shift,seed", [(2.6e6, 300000, 12, 5, 41), (25e6, 250000, 16, 4, 42), (25e6, 70001, 16, 4, 43)])
def test_fill_block_random_vs_oracle(pkg, synth, oracle, fs, nsamp, nch, shift, seed):
    ch = pkg.synth_descriptors(1, nch=nch, seed=seed)[0]
    want, _, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
    want = want[0]
    fmt = pkg.OUT_SC8(shift)
    c0 = clipped(pkg, synth)
    got, _ = synth.fill_block(ch, 1.0 / fs, nsamp, fmt=fmt)
    assert (got == pkg.pack_iq(want, fmt)).all()
    n = clips(want, shift)
    assert clipped(pkg, synth) - c0 == n
    if nch == 16:
        assert n > 0                                      # 16 channels at a shift of 4 do clip: the count is exercised
    if nsamp % 4 == 0:
        got, _ = synth.fill_block(ch, 1.0 / fs, nsamp, fmt=pkg.OUT_SC1)
        assert (got == pkg.pack_iq(want, pkg.OUT_SC1)).all()


def test_fill_block_fixed_carrier(pkg, synth, oracle):
    ch = pkg.synth_descriptors(1, nch=16, seed=44)[0]
    ch["carr_phase"] = np.floor(ch["carr_phase"] * 2.0 ** 32)
    for fs, nsamp in ((25e6, 100000), (2.6e6, 300000)):
        want, _, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp, fixed=True)
        for fmt in (pkg.OUT_SC8(4), pkg.OUT_SC1):
            got, _ = synth.fill_block(ch, 1.0 / fs, nsamp, flags=pkg.FIXED_CARRIER, fmt=fmt)
            assert (got == pkg.pack_iq(want[0], fmt)).all(), (fs, hex(fmt))


def test_fill_block_into_a_registered_buffer(pkg, synth, oracle):
    """the direct path: the packing kernel writes into the registered iq_buff over the bus; nothing around the block is touched.
    At the start of the range, at an odd byte offset (the per-byte path), and straddling its end (copied, as for int16)."""
    L = pkg.lib()
    buf = np.zeros(1 << 21, np.uint8)
    nreg = 1 << 20
    assert L.gpsbb_host_register(synth._h, buf.ctypes.data, nreg) == 0
    try:
        for nch, fs, nsamp, at, fmt, seed in ((12, 2.6e6, 300000, 0, pkg.OUT_SC8(5), 51), (16, 25e6, 200000, 8, pkg.OUT_SC8(4), 52),
                                              (12, 2.6e6, 300000, 333, pkg.OUT_SC8(5), 53), (16, 25e6, 400000, 64, pkg.OUT_SC1, 54),
                                              (12, 2.6e6, 300000, 4097, pkg.OUT_SC1, 55), (12, 2.6e6, 300000, nreg - 1000, pkg.OUT_SC8(5), 56)):
            ch = pkg.synth_descriptors(1, nch=nch, seed=seed)[0]
            want, want_st, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp)
            nb = pkg.out_bytes(fmt, nsamp)
            buf[:] = 0x5A
            c0 = clipped(pkg, synth)
            got, st = synth.fill_block(ch, 1.0 / fs, nsamp, fmt=fmt, out=buf[at:at + nb])
            assert (got == pkg.pack_iq(want[0], fmt)).all(), (at, hex(fmt))
            assert got.ctypes.data == buf.ctypes.data + at
            assert (buf[:at] == 0x5A).all() and (buf[at + nb:] == 0x5A).all()
            assert st["carr_phase"].tobytes() == want_st[0]["carr_phase"].tobytes()
            if fmt != pkg.OUT_SC1:
                assert clipped(pkg, synth) - c0 == clips(want[0], (fmt >> 12) & 15)
    finally:
        assert L.gpsbb_host_unregister(synth._h, buf.ctypes.data) == 0


# ---- the streaming ring -------------------------------------------------------------------------------------------------

def run_stream(pkg, synth, ch, delt, nsamp, bps, depth, fmt, flags=None):
    s = synth.stream(ch.shape[1], delt, nsamp, bps, depth=depth, flags=pkg.CHAIN_CARRIER if flags is None else flags, fmt=fmt)
    out, sts, digs = [], [], []
    npush = ch.shape[0] // bps
    k = 0
    while len(out) < npush:
        while k < npush and s.pending < depth:
            s.push(ch[k * bps:(k + 1) * bps], digest=True)
            k += 1
        iq, st, dg = s.pop_digest()
        out.append(iq)
        sts.append(st)
        digs.append(dg)
    s.close()
    return np.concatenate(out), np.concatenate(sts), np.concatenate(digs)


@pytest.mark.parametrize("fs,nsamp,nch,bps,depth,npush", [(25e6, 250000, 16, 2, 2, 5), (2.6e6, 300000, 12, 3, 3, 4), (4.092e6, 50000, 8, 4, 3, 6)])
def test_chained_stream_packs_every_slot(pkg, synth, oracle, fs, nsamp, nch, bps, depth, npush):
    ch = pkg.synth_descriptors(bps * npush, nch=nch, seed=nsamp + bps)
    iq16, st16, dg16 = run_stream(pkg, synth, ch, 1.0 / fs, nsamp, bps, depth, pkg.OUT_SC16)
    if nch == 8:
        want, _, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp, chain=True)
        assert (iq16 == want).all()
    assert (dg16 == pkg.block_digest_host(iq16)).all()
    for fmt in (pkg.OUT_SC8(4), pkg.OUT_SC8(5), pkg.OUT_SC1):
        c0 = clipped(pkg, synth)
        got, st, dg = run_stream(pkg, synth, ch, 1.0 / fs, nsamp, bps, depth, fmt)
        assert (got == pkg.pack_iq(iq16, fmt)).all(), hex(fmt)
        assert st.tobytes() == st16.tobytes()
        assert (dg == dg16).all()                         # digests are of the int16 render
        assert clipped(pkg, synth) - c0 == (clips(iq16, (fmt >> 12) & 15) if fmt != pkg.OUT_SC1 else 0)


def test_fixed_carrier_stream_sc8(pkg, synth):
    ch = pkg.synth_descriptors(8, nch=16, seed=61)
    ch["carr_phase"] = np.floor(ch["carr_phase"] * 2.0 ** 32)
    fl = pkg.CHAIN_CARRIER | pkg.FIXED_CARRIER
    iq16, st16, _ = run_stream(pkg, synth, ch, 1 / 25e6, 100000, 2, 3, pkg.OUT_SC16, flags=fl)
    got, st, _ = run_stream(pkg, synth, ch, 1 / 25e6, 100000, 2, 3, pkg.OUT_SC8(4), flags=fl)
    assert (got == pkg.pack_iq(iq16, pkg.OUT_SC8(4))).all() and st.tobytes() == st16.tobytes()


# ---- what is refused, and that the handle / stream go on -------------------------------------------------------------

def test_badarg_cases_leave_handle_and_stream_usable(pkg, synth, oracle):
    L = pkg.lib()
    fs, nsamp, nch = 2.6e6, 30000, 12
    ch = pkg.synth_descriptors(4, nch=nch, seed=71)
    want, _, _ = oracle.fill_blocks(ch, 1.0 / fs, nsamp, chain=True)
    good = synth.stream(nch, 1.0 / fs, nsamp, 2, depth=2, flags=pkg.CHAIN_CARRIER, fmt=pkg.OUT_SC8(5))
    good.push(ch[:2])
    st_ = C.c_void_p()
    b_ = C.c_void_p()
    buf = np.zeros(nsamp * 4, np.uint8)
    for fl in (pkg.OUT_SC8(4), pkg.OUT_SC1, pkg.OUT_SC8(16), 3 << 8):
        assert L.gpsbb_batch_create(synth._h, ch.ctypes.data, 1, nch, 1.0 / fs, nsamp, fl, C.byref(b_)) == BADARG
    for fl, n in ((pkg.OUT_SC8(4) | pkg.STREAM_DEVICE_ONLY, nsamp), (pkg.OUT_SC1 | pkg.STREAM_DEVICE_ONLY, nsamp),
                  (pkg.OUT_SC8(16), nsamp), (3 << 8, nsamp), (15 << 8, nsamp), (pkg.OUT_SC1 | 1 << 12, nsamp), (pkg.OUT_SC1, nsamp + 2)):
        assert L.gpsbb_stream_create(synth._h, nch, 1.0 / fs, n, 2, 2, pkg.CHAIN_CARRIER | fl, C.byref(st_)) == BADARG, hex(fl)
        assert not st_.value
    for fl, n in ((pkg.OUT_SC8(16), nsamp), (3 << 8, nsamp), (pkg.OUT_SC1, nsamp + 2), (1 << 12, nsamp)):
        assert L.gpsbb_fill_block_ex(synth._h, ch[0].ctypes.data, nch, 1.0 / fs, n, fl, buf.ctypes.data, None) == BADARG, hex(fl)
    d = on_device(want)
    for fl, n in ((pkg.OUT_SC8(16), nsamp), (7 << 8, nsamp), (pkg.OUT_SC1, nsamp - 2), (pkg.OUT_SC8(4) | pkg.CHAIN_CARRIER, nsamp)):
        assert L.gpsbb_device_pack(synth._h, C.c_void_p(d.data_ptr()), 1, n, fl, buf.ctypes.data) == BADARG, hex(fl)
    # ... and everything goes on: the ring, the fill, a batch, the pack
    good.push(ch[2:4])
    a, _ = good.pop()
    b, _ = good.pop()
    assert (np.concatenate([a, b]) == pkg.pack_iq(want, pkg.OUT_SC8(5))).all()
    good.close()
    got, _ = synth.fill_block(ch[0], 1.0 / fs, nsamp, fmt=pkg.OUT_SC1)
    w0, _, _ = oracle.fill_blocks(ch[0], 1.0 / fs, nsamp)
    assert (got == pkg.pack_iq(w0[0], pkg.OUT_SC1)).all()
    bt = synth.batch(ch[:1], 1.0 / fs, nsamp)
    bt.run()
    synth.sync()
    assert (bt.read()[0] == w0).all()
    assert (synth.device_pack(bt.device_iq(), 1, nsamp, pkg.OUT_SC8(5)) == pkg.pack_iq(w0, pkg.OUT_SC8(5))).all()
    bt.close()


def test_node_refuses_formats_it_cannot_deliver(pkg, synth):
    for fl in (pkg.NODE_DEVICE_ONLY | pkg.OUT_SC8(5), pkg.NODE_DEVICE_ONLY | pkg.OUT_SC1, pkg.OUT_SC8(16), 3 << 8):
        with pytest.raises(pkg.GpsbbError) as e:
            pkg.Node(1, 4, 1 / 2.6e6, 30000, 2, flags=fl, devices=[0])
        assert e.value.rc == BADARG
    with pytest.raises(pkg.GpsbbError) as e:
        pkg.Node(1, 4, 1 / 2.6e6, 30002, 2, fmt=pkg.OUT_SC1, devices=[0])
    assert e.value.rc == BADARG
    ch = pkg.synth_descriptors(4, nch=4, seed=81)
    with pkg.Node(1, 4, 1 / 2.6e6, 30000, 2, devices=[0], fmt=pkg.OUT_SC8(5)) as node:
        with pytest.raises(pkg.GpsbbError):
            node.run_digest(ch)                           # digests are of int16 blocks
        got = np.zeros((4, 30000, 2), np.int8)

        def sink(ptr, first, nb, shard):
            got[first:first + nb] = pkg.iq_view(ptr, nb, 30000, pkg.OUT_SC8(5))
        node.run(ch, sink)
    w, _ = synth.fill_block(ch[0], 1 / 2.6e6, 30000)    # block 0 starts from its own descriptor
    assert (got[0] == pkg.pack_iq(w, pkg.OUT_SC8(5))).all()


# ---- the node driver ----------------------------------------------------------------------------------------------------

def node_run(pkg, ch, fs, nsamp, flags, fmt):
    nblocks = ch.shape[0]
    out = {}
    order = []

    def sink(ptr, first, nb, shard):
        out[first] = pkg.iq_view(ptr, nb, nsamp, fmt).copy()
        order.append(first)
    with pkg.Node(2, ch.shape[1], 1.0 / fs, nsamp, 2, depth=2, flags=flags, devices=[0, 0], fmt=fmt) as node:
        st = node.run(ch, sink)
    assert st["blocks"] == nblocks
    if not flags & pkg.NODE_INDEXED:
        assert order == sorted(order)
    return np.concatenate([out[k] for k in sorted(out)])


@pytest.mark.parametrize("flags", [0, 1])
def test_node_two_shards_pack_like_the_int16_run(pkg, flags):
    fs, nsamp = 25e6, 250000
    ch = pkg.synth_descriptors(10, nch=16, seed=91)
    iq16 = node_run(pkg, ch, fs, nsamp, flags, pkg.OUT_SC16)
    for fmt in (pkg.OUT_SC8(4), pkg.OUT_SC1):
        assert (node_run(pkg, ch, fs, nsamp, flags, fmt) == pkg.pack_iq(iq16, fmt)).all(), (flags, hex(fmt))


# ---- gpsbb-sim ------------------------------------------------------------------------------------------------------------

def sim(pkg, out, *args):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    r = subprocess.run([exe, "-e", os.path.join(GOLDEN, "synth3540.14n"), "-l", "30.286502,120.032669,100", "-s", "2600000",
                        *args, "-o", out], check=True, stderr=subprocess.PIPE, text=True, timeout=600)
    return r.stderr


@pytest.mark.parametrize("path", [["-d", "0.3"], ["-d", "0.3", "-R"], ["-d", "30.1", "-F"], ["-d", "3.2", "-G", "2", "-g", "0,0"]])
def test_gpsbb_sim_writes_packed_files(pkg, tmp_path, path):
    pkg.build_frontend()
    z = np.load(os.path.join(GOLDEN, "static_F.npz"))
    nsamp = int(z["nsamp"])
    plain, b16 = str(tmp_path / "plain.bin"), str(tmp_path / "b16.bin")
    sim(pkg, plain, *path)
    sim(pkg, b16, *path, "-b", "16")
    assert open(plain, "rb").read() == open(b16, "rb").read()
    iq = np.fromfile(b16, np.int16).reshape(-1, nsamp, 2)
    if path[1] == "0.3" or "-F" in path:
        blocks = [int(b) for b in z["blocks"] if b < iq.shape[0]]
        for k, blk in enumerate(blocks):
            assert sha(iq[blk]) == str(z["iq_sha256"][k]), blk
    for args, fmt in ((["-b", "8"], pkg.OUT_SC8(5)), (["-b", "8", "-q", "4"], pkg.OUT_SC8(4)), (["-b", "1"], pkg.OUT_SC1)):
        f = str(tmp_path / ("b%s.bin" % "".join(args)))
        err = sim(pkg, f, *path, *args)
        want = pkg.pack_iq(iq, fmt)
        got = np.fromfile(f, want.dtype).reshape(want.shape)
        assert (got == want).all(), (path, args)
        if fmt != pkg.OUT_SC1 and "-G" not in path:
            n = int(err.split("8-bit components clipped: ")[1].split()[0])
            # (-F renders the short last slot in full: its padding blocks are packed, and counted, but not written)
            assert n == clips(iq, (fmt >> 12) & 15) if "-F" not in path else n >= clips(iq, (fmt >> 12) & 15)
