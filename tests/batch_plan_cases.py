"""The fixed matrix of descriptors behind tests/test_batch_plan.py and tests/golden/batch_plans.json: every case is one set-up (a
resident batch, or the pushes of a ring), named, generated from numpy.random.default_rng(SEED).  cases() yields dicts:
  name, ch [pushes][nblocks, nch] descriptors, delt, nsamp, flags, seed_where, synth_kernel, chain_where,
  stream: None (gpsbb_batch_create) or "carry" / "fixed" / "plain" (a ring of depth 2, one push per entry of ch: the IEEE chain on
  the device, the accumulator's chain on the host, no chain), expect: None or the error code set-up must return."""
import numpy as np

SEED = 20261018
CHAIN, FIXED = 1, 2
FLAGS = (0, CHAIN, FIXED, FIXED | CHAIN)
FS_MIX = 15.5 * 1.023e6 + 20.0  # a run of 15.5 samples holds one chip change where f_code < FS_MIX / 15.5 = 1.023e6 + 1.29 Hz


def descriptors(rng, pkg, nblocks, nch, fixed, max_doppler=5000.0):
    ch = np.zeros((nblocks, nch), pkg.CHAN_DTYPE)
    ch["prn"] = np.arange(1, nch + 1, dtype=np.int32)[None, :]
    ch["f_carr"] = (rng.random((nblocks, nch)) * 2.0 - 1.0) * max_doppler
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    ch["code_phase"] = rng.random((nblocks, nch)) * 1023.0
    ch["carr_phase"] = np.floor(rng.random((nblocks, nch)) * 4294967296.0) if fixed else rng.random((nblocks, nch))
    ch["gain"] = 0.30 + 0.50 * rng.random((nblocks, nch))
    ch["iword"] = rng.integers(9, 59, (nblocks, nch))
    ch["ibit"] = rng.integers(0, 30, (nblocks, nch))
    ch["icode"] = rng.integers(0, 20, (nblocks, nch))
    ch["dwrd"] = rng.integers(0, 1 << 30, (nblocks, nch, pkg.N_DWRD))
    return ch


# geometry name -> (sample rate, samples per block)
GEOMETRIES = {
    "25M": (25e6, 2500000), "2M6": (2.6e6, 300000), "1M": (1e6, 100000), "mix": (FS_MIX, 300000),
    "t1075": (25e6, 1100000), "t1024": (25e6, 1024 * 1024), "t1023": (25e6, 1023 * 1024),
    "t15": (25e6, 15 * 1024), "t16": (25e6, 16 * 1024), "t31": (25e6, 31 * 1024), "t32": (25e6, 32 * 1024), "odd": (2.6e6, 4097),
}


def cases(pkg):
    rng = np.random.default_rng(SEED)
    out = []

    def add(name, ch, geo, flags, seed_where=0, synth_kernel=0, chain_where=0, stream=None, expect=None):
        fs, nsamp = GEOMETRIES[geo] if isinstance(geo, str) else geo
        out.append(dict(name=name, ch=ch if isinstance(ch, list) else [ch], delt=1.0 / fs, nsamp=nsamp, flags=flags,
                        seed_where=seed_where, synth_kernel=synth_kernel, chain_where=chain_where, stream=stream, expect=expect))

    def mixed_dense(ch):
        ch["f_code"] = 1.023e6 + np.where(np.arange(ch.shape[1]) % 2, 3.0, -3.0)[None, :]  # either side of the one-chip limit
        return ch

    # geometries x sizes (64 against 80 block-channels: HOST_SEED_MAX_CHANNELS) x flags x {library's choice, row walks}
    for geo in GEOMETRIES:
        for nblocks in (1, 4, 5):
            for flags in FLAGS:
                ch = descriptors(rng, pkg, nblocks, 16, bool(flags & FIXED))
                if geo == "mix":
                    mixed_dense(ch)
                for sw in (0, 1):
                    add("geo-%s-%dx16-f%d-sw%d" % (geo, nblocks, flags, sw), ch, geo, flags, seed_where=sw)
    # every option value, on 80 block-channels of the reference's geometry and on 64
    for flags in FLAGS:
        ch5 = descriptors(rng, pkg, 5, 16, bool(flags & FIXED))
        for sw in range(4):
            for cw in range(4):
                for sk in (0, 1):
                    add("opt-5x16-f%d-sw%d-cw%d-sk%d" % (flags, sw, cw, sk), ch5, "2M6", flags, sw, sk, cw)
        ch4 = descriptors(rng, pkg, 4, 16, bool(flags & FIXED))
        for sw in range(4):
            for sk in (0, 1):
                add("opt-4x16-f%d-sw%d-sk%d" % (flags, sw, sk), ch4, "2M6", flags, sw, sk, 0)
    # 400 blocks
    for flags in FLAGS:
        ch = descriptors(rng, pkg, 400, 16, bool(flags & FIXED))
        for sw, sk in ((0, 0), (1, 0), (1, 1)):
            add("big-2M6-400x16-f%d-sw%d-sk%d" % (flags, sw, sk), ch, "2M6", flags, sw, sk)
    ch = descriptors(rng, pkg, 400, 16, False)
    add("big-25M-400x16-f1-sw0", ch, "25M", CHAIN)
    add("big-25M-400x16-f1-sw1", ch, "25M", CHAIN, seed_where=1)
    add("big-25M-400x16-f0-sw1", ch, "25M", 0, seed_where=1)
    add("big-mix-400x16-f0", mixed_dense(descriptors(rng, pkg, 400, 16, False)), "mix", 0)
    # nblocks * nseg either side of 2048 (FIXP_WG_ALONE) and 4096 (CHAIN_MODEL_MAX_SEGS): one channel whose carrier step of 0.01
    # cycles per sample makes two segments of a 32-tile block (the row walks: seed_where 1)
    for nblocks in (1023, 1024, 2048, 2049):
        ch = descriptors(rng, pkg, nblocks, 1, False)
        ch["f_carr"] = 0.01 * 25e6 * (1.0 + 0.001 * rng.random((nblocks, 1)))
        add("segs-%dx1-chain" % nblocks, ch, "t32", CHAIN, seed_where=1)
        add("segs-%dx1-indep" % nblocks, ch, "t1024", 0, seed_where=1)
    # channel contents, on 80 block-channels of the reference's geometry
    def contents(name, edit, fixed_too=True):
        for flags in FLAGS if fixed_too else (0, CHAIN):
            ch = edit(descriptors(rng, pkg, 5, 16, bool(flags & FIXED)))
            for sw in (0, 1):
                add("ch-%s-f%d-sw%d" % (name, flags, sw), ch, "2M6", flags, seed_where=sw)

    def idle(ch):
        ch["prn"][:, 3] = 0
        ch["prn"][:, 15] = 0
        ch["prn"][2, 7] = 0  # one block only: the chain of channel 7 starts again behind it
        return ch

    def zero_carrier(ch):
        ch["f_carr"][:, 5] = 0.0
        return ch

    def negative(ch):
        ch["f_carr"] = -np.abs(ch["f_carr"])
        return ch

    def tiny(ch):
        ch["f_carr"][:, 2] = 1e-10  # |f_carr * delt| = 3.8e-17 < 2^-50: the laps decline
        return ch

    def gains(total):
        def edit(ch):
            ch["gain"] = (total - 16.0) / 512.0 / 16.0  # sum over 16 channels of 512 |gain| + 1 = total
            return ch
        return edit

    contents("idle", idle)
    contents("zero", zero_carrier)
    contents("neg", negative)
    contents("tiny", tiny, fixed_too=False)
    contents("gain-under", gains(32767.5))
    contents("gain-over", gains(32768.5))
    # a ring's pushes.  carry: the IEEE chain on the device (80 block-channels: whatever the pre-pass; 8: where the laps take it)
    def pushes(nblocks, nch, fixed, swap):
        p = [descriptors(rng, pkg, nblocks, nch, fixed) for _ in range(3)]
        if swap:
            p[2]["prn"][:, 1] = 31  # the third push: one PRN swapped (cont0_mask)
        return p

    for sw, sk in ((0, 0), (1, 0), (3, 0), (0, 1), (1, 1)):
        add("ring-carry-5x16-sw%d-sk%d" % (sw, sk), pushes(5, 16, False, True), "2M6", CHAIN, sw, sk, stream="carry")
    add("ring-carry-2x4", pushes(2, 4, False, True), (25e6, 4096), CHAIN, stream="carry")
    for sw in (0, 1):
        add("ring-fixed-5x16-sw%d" % sw, pushes(5, 16, True, True), "2M6", FIXED | CHAIN, sw, stream="fixed")
        add("ring-plain-5x16-sw%d" % sw, pushes(5, 16, False, False), "2M6", 0, sw, stream="plain")
    add("ring-plain-fixed-5x16", pushes(5, 16, True, False), "2M6", FIXED, stream="plain")
    # errors: where set-up returns them
    bad = descriptors(rng, pkg, 2, 16, False)
    bad["prn"][1, 4] = 33
    add("err-badchan", bad, "2M6", 0, expect=-2)
    add("err-badarg-flags", descriptors(rng, pkg, 2, 16, False), "2M6", 4, expect=-1)
    big = np.zeros((4096, 16), pkg.CHAN_DTYPE)  # 2 * 65536 * (32767 + 1) tile-index entries = 2^32: the first count refused
    add("err-nomem-tiles", big, (25e6, 32767 * 1024), 0, expect=-4)
    return out


def fixed_chain_state(ch, delt, nsamp, chained, prev_prn, prev_phase):
    """The accumulator's state behind the last block of a push (what gpsbb_stream_push keeps for the next): prn and phase per
    channel, from the push's descriptors and the state before it (None: a first push)."""
    nb, nch = ch.shape
    prn = np.zeros(nch, np.int32)
    phase = np.zeros(nch, np.uint32)
    for i in range(nch):
        pp = int(prev_prn[i]) if prev_prn is not None else 0
        ph = int(prev_phase[i]) if prev_phase is not None else 0
        k0 = step = 0
        for b in range(nb):
            c = ch[b, i]
            if c["prn"] <= 0:
                pp = 0
                k0 = step = 0
                continue
            x = 512.0 * 65536.0 * float(c["f_carr"]) * delt
            step = int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)  # std::round
            k0 = ph if (chained and int(c["prn"]) == pp) else int(c["carr_phase"])
            ph = (k0 + nsamp * step) & 0xFFFFFFFF
            pp = int(c["prn"])
        last = ch[nb - 1, i]
        prn[i] = last["prn"] if last["prn"] > 0 else 0
        phase[i] = (k0 + nsamp * step) & 0xFFFFFFFF
    return prn, phase


def write_matrix(pkg, path):
    """The matrix as tools/plan_asan.cpp reads it: per set-up a Record (see there), then the descriptors."""
    rec = np.dtype([("nblocks", "<i4"), ("nch", "<i4"), ("nsamp", "<i4"), ("first", "<i4"), ("opt", "<i4", 5), ("carry", "<i4"),
                    ("fixed_prev", "<i4"), ("carry_prn", "<i4", 16), ("fx_prn", "<i4", 16), ("flags", "<u4"), ("fx_phase", "<u4", 16),
                    ("delt", "<f8")])
    with open(path, "wb") as f:
        for c in cases(pkg):
            prn, fx = np.zeros(16, np.int32), None
            for k, ch in enumerate(c["ch"]):
                r = np.zeros(1, rec)
                r["nblocks"], r["nch"] = ch.shape
                r["nsamp"], r["first"], r["flags"], r["delt"] = c["nsamp"], k == 0, c["flags"], c["delt"]
                r["opt"] = (c["seed_where"], c["synth_kernel"], 0, c["chain_where"], 6 if c["stream"] is None else 1)
                r["carry"], r["carry_prn"] = c["stream"] == "carry", prn
                if c["stream"] == "fixed" and fx is not None:
                    r["fixed_prev"], r["fx_prn"], r["fx_phase"] = 1, np.resize(fx[0], 16), np.resize(fx[1], 16)
                f.write(r.tobytes())
                f.write(np.ascontiguousarray(ch).tobytes())
                prn[:ch.shape[1]] = np.maximum(ch["prn"][-1], 0)
                if c["stream"] == "fixed":
                    fx = fixed_chain_state(ch, c["delt"], c["nsamp"], True, *(fx or (None, None)))


if __name__ == "__main__":
    import sys
    from conftest import load_package
    write_matrix(load_package(), sys.argv[1])
