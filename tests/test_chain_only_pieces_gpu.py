"""gpsbb_chain_carrier across its sub-batch boundaries, on the device: the carry from piece to piece, cont0_mask of a piece's first
block, a PRN that changes or goes idle on the boundary (tests/test_chain_plan.py holds the plan of the same call to the record
without a GPU).  The experiments build with the sub-batch limits lowered to 16 blocks and 2000 laps cuts the 50 blocks x 5 channels
of tests/chain_plan_cases.py's boundary case into four pieces; one child process per pre-pass (the limits are read once): the
lap-parallel one, and the row walks (GPSBB_OPT_SEED_WHERE 1).  Each child holds the device's phases to gpsbb_chain_carrier_host's,
bit for bit, and asks gpsbb_test_chain_plan that the call did take that path in at least three pieces."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def child(pkg, cpc, where):
    ch, delt, nsamp = cpc.edge_descriptors(pkg), 1.0 / cpc.FS, cpc.EDGE_NSAMP
    rc, plan = pkg.chain_plan(ch, delt, nsamp, where)
    assert rc == 0 and plan["laps"] == int(where != 1) and plan["npieces"] >= 3, plan
    assert [p[0] for p in plan["pieces"]] == [0, 16, 32, 48]
    longer = np.concatenate([ch, ch[-1:]])  # one appended block: where it starts is where the last one ended
    want = pkg.chain_carrier_host(longer, delt, nsamp)
    assert (ch["prn"][-1] > 0).all()
    with pkg.Synth(0) as s:
        s.set_option(pkg.OPT_SEED_WHERE, where)
        seeds, end = s.chain_carrier(ch, delt, nsamp)
        assert s.info(pkg.INFO_CHAIN_ON_DEVICE) == 1
        assert seeds.tobytes() == want[:-1].tobytes(), "start phases: %d differ" % np.count_nonzero(seeds != want[:-1])
        assert end.tobytes() == want[-1].tobytes(), "end phases"
        _, end_only = s.chain_carrier(ch, delt, nsamp, want_seeds=False)
        assert end_only.tobytes() == want[-1].tobytes(), "end phases of a call without seeds"
        assert s.shard_seed(ch, 20, delt, nsamp).tobytes() == want[20].tobytes(), "shard seed inside the second piece"
        seeds, end = s.chain_carrier(ch[:35], delt, nsamp)  # the same handle's scratch, fewer blocks: pieces of 16, 16 and 3
        assert seeds.tobytes() == want[:35].tobytes() and end.tobytes() == want[35].tobytes(), "a second, shorter call"
    print("pieces ok: where %d, %d pieces" % (where, plan["npieces"]))


def test_chain_alone_is_exact_across_its_pieces(pkg):
    import chain_plan_cases as cpc
    env = dict(os.environ, GPSBB_PY_LIB="exp", **cpc.LOWERED)
    for where in (0, 1):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(where)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "pieces ok: where %d" % where in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from conftest import load_package
    import chain_plan_cases
    child(load_package(), chain_plan_cases, int(sys.argv[1]))
