"""Everything the library makes, it frees.  Device buffers, pinned host buffers and HIP events each have one owner type in gpsbb.hip
(DevBuf, PinnedBuf, Event) that counts what is live (gpsbb_test_live).  One cycle here creates a handle of its own, makes every
lazily created resource exist, closes everything in the order the header allows (batches and streams before their handle) and
must find all three counts where they were; a second cycle must do so again and give the first one's results, byte for byte.
The shapes are the smallest the project has: the small cases of tools/*_check.py and 3 channels over blocks of 4000 samples."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402
import fir_check as fc  # noqa: E402
import track_check as tc  # noqa: E402

DELT, NSAMP, NCH, BPS = 1.0 / 2.6e6, 4000, 3, 2


def live(pkg):
    out = (C.c_longlong * 3)()
    pkg.lib().gpsbb_test_live(out)
    return list(out)


def flat(x):
    """the bytes of a result: an array or a number, or a tuple / list of results"""
    return b"".join(flat(v) for v in x) if isinstance(x, (tuple, list)) else np.ascontiguousarray(x).tobytes()


def batch_results(pkg, s, ch, despread=False):
    """a chained batch run three times, read, and closed"""
    b = s.batch(ch, DELT, NSAMP, flags=pkg.CHAIN_CARRIER)
    try:
        for _ in range(3):
            b.run()
        s.sync()
        out = [b.read(), b.despread() if despread else 0]
        return out, (s.info(pkg.INFO_LAST_KERNEL), s.info(pkg.INFO_PREPASS))
    finally:
        b.close()


def stream_results(pkg, s, ch):
    """a depth-2 ring of four pushes, every slot once with its digests and once with its level"""
    st = s.stream(NCH, DELT, NSAMP, BPS, depth=2, flags=pkg.CHAIN_CARRIER)
    try:
        out = []
        for k, (first, second) in enumerate(((st.pop_digest, st.pop_level), (st.pop_level, st.pop_digest))):
            st.push(ch[2 * k * BPS:(2 * k + 1) * BPS], digest=k == 0, level=k == 1)
            st.push(ch[(2 * k + 1) * BPS:(2 * k + 2) * BPS], digest=k == 1, level=k == 0)
            out += [first(), second()]
        return out, s.info(pkg.INFO_CHAIN_ON_DEVICE)
    finally:
        st.close()


def cycle(pkg, inputs):
    """one life of a handle -> (every result as bytes, in a fixed order; what each fill added to the live counts, then which
    paths the batches and the rings took)"""
    import torch
    ch = pkg.synth_descriptors(4 * BPS, nch=NCH, seed=0x11FE)
    out, took = [], []
    s = pkg.Synth(0)
    try:
        seen = [live(pkg)]
        # the drop-in call: into a buffer of its own (h_fill), into one that straddles the end of a registered range (h_bounce), and
        # packed with noise (d_pack, the knot table and its clip count)
        buf = np.zeros((3 * NSAMP, 2), np.int16)
        s.host_register(buf[:NSAMP])
        try:
            for kw in ({}, {"out": buf[NSAMP // 2:]}, {"fmt": pkg.OUT_SC8(5), "noise": ac.NOISE}):
                out.append(s.fill_block(ch[0], DELT, NSAMP, **kw))
                seen.append(live(pkg))
        finally:
            s.host_unregister(buf[:NSAMP])
        grew = [[a - b for a, b in zip(now, was)] for was, now in zip(seen, seen[1:])]
        took.append([grew[0][1:], grew[1], grew[2]])
        # batches: pre-pass on the device, then on host threads for the breakpoint kernel and for the per-sample kernel
        for seed_where, synth_kernel in ((0, 0), (2, 0), (2, 1)):
            s.set_option(pkg.OPT_SEED_WHERE, seed_where)
            s.set_option(pkg.OPT_SYNTH_KERNEL, synth_kernel)
            res, path = batch_results(pkg, s, ch[:3], despread=seed_where == 0)
            out.append(res)
            took.append(path)
        s.set_option(pkg.OPT_SEED_WHERE, 0)
        s.set_option(pkg.OPT_SYNTH_KERNEL, 0)
        # rings: the carrier chained on the device, then on host threads
        for chain_where in (0, 1):
            s.set_option(pkg.OPT_CHAIN_WHERE, chain_where)
            res, path = stream_results(pkg, s, ch)
            out.append(res)
            took.append(path)
        s.set_option(pkg.OPT_CHAIN_WHERE, 0)
        out.append(s.chain_carrier(ch, DELT, NSAMP))
        # the calls that read device IQ
        p = {k: v.data_ptr() for k, v in inputs["dev"].items()}
        out.append(s.device_level(p["blocks"], 3, 1024))
        out.append(s.device_digest(p["blocks"], 3, 1024))
        out.append(s.device_acquire(p["acq"], inputs["acq"][0].shape[0], inputs["acq"][1], want_grid=True))
        out.append(s.device_track(p["trk"], inputs["trk"][0].shape[0], inputs["trk"][1], inputs["trk"][2]))
        fir_out = torch.zeros((1024, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        out.append(s.device_fir(p["blocks"], 4096, fc.random_fir(pkg, 33, 4, 12, 0xF16), fir_out.data_ptr()))
        out.append(fir_out.cpu().numpy())
    finally:
        s.close()
    return [flat(r) for r in out], took


@pytest.mark.gpu
def test_two_lives_of_a_handle_leave_nothing_and_agree(pkg):
    import torch
    # the paths the cycle means to take are the ones these shapes do take (the plans, without a GPU)
    ch = pkg.synth_descriptors(4 * BPS, nch=NCH, seed=0x11FE)
    plans = [pkg.plan(ch[:3], DELT, NSAMP, flags=pkg.CHAIN_CARRIER, seed_where=w, synth_kernel=k)[1] for w, k in ((0, 0), (2, 0), (2, 1))]
    assert [(q["host_seed"], q["ev"]) for q in plans] == [(0, 1), (1, 1), (1, 0)] and plans[0]["chain_dev"] == 1
    sides = [pkg.push_side(ch[:BPS], DELT, NSAMP, flags=pkg.CHAIN_CARRIER, chain_where=w)[1]["chain"] for w in (0, 1)]
    assert sides == [pkg.PUSH_CHAIN_DEVICE, pkg.PUSH_CHAIN_HOST]
    acq_iq, acq_cfg = ac.lane_map_case(pkg)
    trk = tc.ends_case(pkg)
    host = {"blocks": ac.random_iq(4096, 0x1E7), "acq": acq_iq, "trk": trk[0]}
    inputs = {"acq": (acq_iq, acq_cfg), "trk": trk,
              "dev": {k: torch.from_numpy(np.ascontiguousarray(v, np.int16)).cuda() for k, v in host.items()}}
    torch.cuda.synchronize()
    before = live(pkg)
    first, took = cycle(pkg, inputs)
    after_first = live(pkg)
    second, took_again = cycle(pkg, inputs)
    after_second = live(pkg)
    assert after_first == before, "a handle's life left (device buffers, pinned buffers, events) %s, was %s" % (after_first, before)
    assert after_second == before
    assert len(first) == len(second) == 15
    assert [k for k, (a, b) in enumerate(zip(first, second)) if a != b] == []
    # What each fill added to (device buffers, pinned buffers, events).  The first: the scratch batch's tables (not counted here), the
    # pinned stage and h_fill, the event upload_done (a one-stream batch makes no timing events).  The straddling one: h_bounce and
    # nothing else, the batch is set up already.  The packed one with noise: d_pack, the knot table and its clip count.  Then (last
    # kernel: 2 breakpoint, 1 per-sample; pre-pass: 3 lap-parallel on the device, 2 host threads) per batch, then the rings' chain side
    assert took == took_again == [[[2, 1], [0, 1, 0], [3, 0, 0]], (2, 3), (2, 2), (1, 2), 1, 0]
