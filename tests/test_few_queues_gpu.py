"""The ordering contract of DESIGN 4.1 at HIP's default of four hardware queues and at twelve.

Which streams share a hardware queue is decided when the runtime starts, from GPU_MAX_HW_QUEUES in the process
environment, so every case runs in a FRESH child process (this file, run as a script) with that variable set.  The
children check ordering, not speed: a chained device-only ring whose every slot is reused three times, chained rings with
host-bound output (int16 and a packed format), and re-runs of resident batches that go round their table sets — IQ, end
states and digests against the CPU oracle, bit for bit.  Every push of a ring has descriptors of its own, so a slot or
a table set taken over too early cannot reproduce the right bytes by accident."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, NSAMP, NCH = 25e6, 12000, 16  # 25 MS/s: k_synth_ev behind the lap-parallel pre-pass


def _load():
    """what tests/conftest.py does for the session, for a process of its own"""
    import importlib.util
    try:  # torch bundles its own libamdhip64: import it BEFORE libgpsbb.so is loaded so both share one HIP runtime
        import torch  # noqa: F401
    except Exception:
        pass
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    spec = importlib.util.spec_from_file_location("pluto_gps_sim_amd", os.path.join(ROOT, "pluto-gps-sim_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["pluto_gps_sim_amd"] = pkg
    spec.loader.exec_module(pkg)
    import oracle_binding as ob
    return pkg, ob.Oracle()


def _ring(pkg, synth, ch, want_iq, want_st, bps, depth, device_only, fmt):
    """Push ch through a chained ring that is kept full, every push with its digests; returns what was checked."""
    import numpy as np
    delt = 1.0 / FS
    npush = ch.shape[0] // bps
    want_dig = pkg.block_digest_host(want_iq)
    st = synth.stream(NCH, delt, NSAMP, bps, depth=depth, flags=pkg.CHAIN_CARRIER | (pkg.STREAM_DEVICE_ONLY if device_only else 0), fmt=fmt)
    pushed = popped = same_slot = 0
    while popped < npush:
        while pushed < npush and st.pending < depth:
            st.push(ch[pushed * bps:(pushed + 1) * bps], digest=True)
            pushed += 1
        assert synth.info(pkg.INFO_PREPASS) == 3, "the lap-parallel pre-pass did not take the push"
        iq, es, dig = st.pop_digest(copy=True)
        lo, hi = popped * bps, (popped + 1) * bps
        assert (dig == want_dig[lo:hi]).all(), ("digest of push", popped)
        if device_only:
            got = synth.device_read(iq, (bps, NSAMP, 2))
            assert (got == want_iq[lo:hi]).all(), ("IQ of push", popped)
            if pushed == npush:  # nothing more to keep in flight (the call waits for the whole handle): the slot's own digests
                assert (synth.device_digest(iq, bps, NSAMP) == dig).all(), ("device digest of push", popped)
                same_slot += 1
        else:
            assert (iq == pkg.pack_iq(want_iq[lo:hi], fmt)).all(), ("host IQ of push", popped, hex(fmt))
        assert es.tobytes() == want_st[lo:hi].tobytes(), ("end states of push", popped)
        popped += 1
    st.close()
    return {"pushes": npush, "slot_digests": same_slot}


def child():
    import numpy as np
    pkg, oracle = _load()
    delt = 1.0 / FS
    out = {"env": os.environ.get("GPU_MAX_HW_QUEUES")}
    with pkg.Synth(0) as synth:
        out["hw_queues"] = synth.info(pkg.INFO_HW_QUEUES)
        # 1. the timed mode of bench.py in small: device-only, depth 6, 3 x depth + 2 pushes
        bps, depth = 3, 6
        ch = pkg.synth_descriptors(bps * (3 * depth + 2), nch=NCH, seed=0xF00)
        want_iq, want_st, _ = oracle.fill_blocks(ch, delt, NSAMP, chain=True)
        out["device_only"] = _ring(pkg, synth, ch, want_iq, want_st, bps, depth, True, pkg.OUT_SC16)
        out["streams_device_only"] = synth.info(pkg.INFO_STREAMS)
        # 2. host-bound output: int16 and 8-bit packed, depth 3, four rounds of the ring
        bps, depth = 2, 3
        ch = pkg.synth_descriptors(bps * 4 * depth, nch=NCH, seed=0xF01)
        want_iq, want_st, _ = oracle.fill_blocks(ch, delt, NSAMP, chain=True)
        for name, fmt in (("sc16", pkg.OUT_SC16), ("sc8", pkg.OUT_SC8(4))):
            out["host_" + name] = _ring(pkg, synth, ch, want_iq, want_st, bps, depth, False, fmt)
        out["streams_host_bound"] = synth.info(pkg.INFO_STREAMS)
        # 3. resident batches re-run: independent blocks (three table sets) and the chained carrier, two batches side by side
        # (created one after the other: they start on different pre-pass streams), seven runs each into buffers of their own
        import torch
        runs = 7
        cases = []
        for k, flags in enumerate((0, pkg.CHAIN_CARRIER)):
            chb = pkg.synth_descriptors(4, nch=NCH, seed=0xF10 + k)
            w_iq, w_st, _ = oracle.fill_blocks(chb, delt, NSAMP, chain=bool(flags))
            cases.append((synth.batch(chb, delt, NSAMP, flags=flags), w_iq, w_st,
                          [torch.zeros((4, NSAMP, 2), dtype=torch.int16, device="cuda:0") for _ in range(runs)]))
        torch.cuda.synchronize()
        for r in range(runs):
            for b, _, _, bufs in cases:
                b.run(bufs[r].data_ptr())
        synth.sync()
        for b, w_iq, w_st, bufs in cases:
            for r in range(runs):
                assert (bufs[r].cpu().numpy() == w_iq).all(), ("batch run", r)
            _, st = b.read(want_iq=False)
            assert st.tobytes() == w_st.tobytes()
            assert synth.info(pkg.INFO_PREPASS) == 3
            b.close()
        out["batch_runs"] = runs * len(cases)
        out["streams_end"] = synth.info(pkg.INFO_STREAMS)
    print(json.dumps(out))


@pytest.mark.gpu
@pytest.mark.parametrize("queues", [4, 12])
def test_rings_and_batches_keep_their_order(pkg, queues):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(queues))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["env"] == str(queues) and out["hw_queues"] == queues
    assert out["device_only"] == {"pushes": 20, "slot_digests": 6}
    assert out["host_sc16"]["pushes"] == out["host_sc8"]["pushes"] == 12 and out["batch_runs"] == 14
    # the steady state of a device-only ring: synthesis, two pre-passes and the process's null stream — HIP's default of four
    # queues; host-bound output adds the copy stream, and nothing creates more
    assert out["streams_device_only"] == 4 and out["streams_host_bound"] == out["streams_end"] == 5


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
