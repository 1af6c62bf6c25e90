"""What the handle reports after a run is what gpsbb_test_launch_plan said the run would be (tests/test_launch_plan.py checks the plan
itself, without a GPU): the synthesis kernel and its variant, the pre-pass, where the chain was resolved — one tiny batch per kind of
launch — and the model kernels render every tile of every block once, which a wrong grid or chunk size would break first."""
import numpy as np
import pytest

import batch_plan_cases as bpc

pytestmark = pytest.mark.gpu

NBLOCKS, NSAMP, NTILES = 2, 3 * 1024 + 5, 4  # three tiles and a partial one
PD_WIDE_CHAN = 12  # csrc/gpsbb_dense.hip.h

# name, sample rate, channels, flags, GPSBB_OPT_SEED_WHERE, GPSBB_OPT_CHAIN_WHERE, a ring's push with digests, the variant expected
SETUPS = [
    ("ev", 25e6, 2, 0, 0, 0, False, "VARIANT_EV"),
    ("ev-digest", 25e6, 2, 0, 0, 0, True, "VARIANT_EV"),
    ("pd-wide", 2.6e6, 2, 0, 0, 0, False, "VARIANT_PD_WIDE"),
    ("pd-narrow", 2.6e6, PD_WIDE_CHAN + 1, 0, 0, 0, False, "VARIANT_PD_NARROW"),
    ("mixed-dense", bpc.FS_MIX, 2, 0, 0, 0, False, "VARIANT_EV_DENSE"),
    ("fixed", 25e6, 2, bpc.FIXED, 0, 0, False, "VARIANT_EV_FIXED"),
    ("per-sample", 1e6, 2, 0, 0, 0, False, "VARIANT_SYNTH"),
    ("row-walks", 25e6, 2, 0, 1, 0, False, "VARIANT_EV"),
    ("host-seed", 25e6, 2, 0, 2, 0, False, "VARIANT_EV"),
    ("chain", 25e6, 2, bpc.CHAIN, 0, 0, False, "VARIANT_EV"),
    ("chain-fix-seq", 25e6, 2, bpc.CHAIN, 0, 2, False, "VARIANT_EV"),
    ("chain-fix-seq-walks", 25e6, 2, bpc.CHAIN, 1, 2, False, "VARIANT_EV"),
]


@pytest.mark.parametrize("setup", SETUPS, ids=[s[0] for s in SETUPS])
def test_a_run_is_what_its_launch_plan_says(pkg, synth, setup):
    import torch
    name, fs, nch, flags, seed_where, chain_where, ring_digest, variant = setup
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(bpc.SEED)
    ch = bpc.descriptors(rng, pkg, NBLOCKS, nch, bool(flags & bpc.FIXED))
    if name == "mixed-dense":
        ch["f_code"] = 1.023e6 + np.where(np.arange(nch) % 2, 3.0, -3.0)[None, :]  # either side of the one-chip limit
    delt = 1.0 / fs
    rc, want = pkg.launch_plan(ch, delt, NSAMP, flags, cus=cus, want_digest=int(ring_digest), seed_where=seed_where,
                               chain_where=chain_where, max_sets=1 if ring_digest else 6)
    assert rc == 0 and want["variant"] == getattr(pkg, variant), (name, want)
    synth.sync()
    tiles0 = synth.info(pkg.INFO_TILES_RENDERED)
    synth.set_option(pkg.OPT_SEED_WHERE, seed_where)
    synth.set_option(pkg.OPT_CHAIN_WHERE, chain_where)
    try:
        if ring_digest:
            st = synth.stream(nch, delt, NSAMP, NBLOCKS, depth=2, flags=flags)
            try:
                st.push(ch, digest=True)
                st.pop_digest()
            finally:
                st.close()
        else:
            b = synth.batch(ch, delt, NSAMP, flags=flags)
            try:
                b.run()
                synth.sync()
            finally:
                b.close()
        synth.sync()
        got = {"last_kernel": synth.info(pkg.INFO_LAST_KERNEL), "variant": synth.info(pkg.INFO_LAST_VARIANT),
               "info_prepass": synth.info(pkg.INFO_PREPASS), "last_chain_dev": synth.info(pkg.INFO_CHAIN_ON_DEVICE)}
        tiles = synth.info(pkg.INFO_TILES_RENDERED) - tiles0
    finally:
        synth.set_option(pkg.OPT_SEED_WHERE, 0)
        synth.set_option(pkg.OPT_CHAIN_WHERE, 0)
    assert got == {k: want[k] for k in got}, (name, got, want)
    if want["variant"] != pkg.VARIANT_SYNTH:
        assert tiles == NBLOCKS * NTILES, (name, tiles)
