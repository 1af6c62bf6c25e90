"""gpsbb_batch_despread_lags against the numpy restatement (despread_lags_host over view_host) fed with the CPU oracle's replicas,
as tools/despread_check.py does it for the prompt sums.  tests/test_despread_lags_gpu.py imports the cases and the comparison
from here; run as a script it checks the cases on one pre-pass and prints how many samples took the kernel's exact path:

    python tools/despread_lags_check.py [--where 0|1]
    GPSBB_PY_LIB=exp GPSBB_DS_DANGER=4194304 python tools/despread_lags_check.py    (the exact path made common)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import despread_check as dc  # noqa: E402

C_LIGHT = 2.99792458e8
SITE = (30.286502, 120.032669, 100.0)
NAV = os.path.join(ROOT, "tests", "golden", "synth3540.14n")
# both ends of the range, both signs next to 0, 0 itself not first, unsorted
LAGS = (-64, -3, -1, 0, 1, 2, 64, 5)
NOISE = {"seed": 0xC0FFEE, "sample0": (1 << 33) + 12345, "sigma": 900.0, "shift": 1}   # sample0 far up and odd


def echo_descriptors(pkg, nblocks, fs, max_chan=11, delay=3, idle=4):
    """descriptors of the golden scenario's first blocks with max_chan satellites' slots and one echo, of the satellite in slot 0,
    `delay` samples late and 6 dB down, a quarter cycle off; slot `idle` emptied -> (descriptors [nblocks, max_chan + 1], prn)"""
    pkg.build_frontend()
    fe = pkg.FrontEnd(NAV, llh=SITE, max_chan=max_chan)
    prn = int(fe.generate(1)["prn"][0, 0])
    fe.close()
    fe = pkg.FrontEnd(NAV, llh=SITE, max_chan=max_chan)
    fe.set_echoes([(prn, delay * C_LIGHT / fs, 6.0, 0.25)])
    ch = fe.generate(nblocks)
    fe.close()
    assert (ch["prn"][:, 0] == prn).all() and (ch["prn"][:, max_chan] == prn).all()
    if idle is not None:
        ch["prn"][:, idle] = 0
    return ch, prn


def cases(pkg):
    """the smallest shapes at which the kernel can go wrong: name -> fs, nsamp, descriptors, the kernel that renders them"""
    out = {}
    # k_synth_pd: 12 slots, one idle, one PRN twice (a direct channel and its echo from gpsfe); a ragged fourth tile; 2 chained blocks
    ch, _ = echo_descriptors(pkg, 2, 2.6e6)
    out["pd"] = dict(fs=2.6e6, nsamp=3 * 1024 + 37, ch=ch, variant=dc.PD_WIDE)
    # k_synth_ev behind the lap pre-pass, one state per two tiles: six tiles, the last 37 samples long (every state serves two),
    # and five, where the last state serves one tile alone.  (Batches this small get their tiles one at a time, one to a
    # wavefront: what a wavefront does from its second tile on is tests/test_despread_lags_gpu.py's large batch.)
    out["ev"] = dict(fs=25e6, nsamp=5 * 1024 + 37, ch=pkg.synth_descriptors(2, nch=16, seed=21), variant=dc.EV)
    out["ev_odd"] = dict(fs=25e6, nsamp=4 * 1024 + 37, ch=pkg.synth_descriptors(2, nch=16, seed=23), variant=dc.EV)
    # shorter than a wavefront and than the largest lag
    out["tiny"] = dict(fs=2.6e6, nsamp=40, ch=pkg.synth_descriptors(1, nch=4, seed=22), variant=dc.PD_WIDE)
    for g in out.values():
        g["delt"] = 1.0 / g["fs"]
    return out


def with_oracle(oracle, g):
    """the oracle's chained render and replicas of a case, added to it"""
    if "iq" not in g:
        g["iq"] = oracle.fill_blocks(g["ch"], g["delt"], g["nsamp"], chain=True)[0]
        g["rep"] = dc.replicas(oracle, g["ch"], g["delt"], g["nsamp"], chain=True)
    return g


def check_batch(pkg, b, iq, rep, seg_tiles_list, lags=LAGS, views=((0, None, None),), d_iq=None):
    """findings (strings) of one run batch: its sums at the lags for every seg_tiles and (view, noise, interf) against the host's"""
    bad = []
    for view, noise, interf in views:
        u = pkg.view_host(iq, view, noise, interf=interf)
        for st in seg_tiles_list:
            got = b.despread_lags(lags, seg_tiles=st, view=view, noise=noise, interf=interf, d_iq=d_iq)
            want = pkg.despread_lags_host(u, rep, st, lags)
            if got.shape != want.shape or not (got == want).all():
                w = np.argwhere(got != want) if got.shape == want.shape else []
                bad.append("view 0x%x noise %s interf %s seg_tiles %d: %d sums differ, first (block, channel, segment, lag, i/q) %s"
                           % (view, noise is not None, interf is not None, st, len(w), w[0].tolist() if len(w) else "shape"))
    return bad


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import torch  # noqa: F401  (one HIP runtime for torch and libgpsbb)
    except Exception:
        pass
    from __graft_entry__ import load_package
    import oracle_binding as ob
    pkg = load_package()
    oracle = ob.Oracle()
    where = int(sys.argv[sys.argv.index("--where") + 1]) if "--where" in sys.argv else 0
    views = [(pkg.OUT_SC16, None, None), (pkg.OUT_SC8(5), NOISE, None)]
    exact = 0
    with pkg.Synth(0) as s:
        s.set_option(pkg.OPT_SEED_WHERE, where)
        for name, g in cases(pkg).items():
            with_oracle(oracle, g)
            b = s.batch(g["ch"], g["delt"], g["nsamp"], flags=pkg.CHAIN_CARRIER)
            b.run()
            s.sync()
            assert s.info(pkg.INFO_LAST_VARIANT) == g["variant"], (name, s.info(pkg.INFO_LAST_VARIANT))
            bad = check_batch(pkg, b, g["iq"], g["rep"], (1, 2), views=views)
            if os.environ.get("GPSBB_PY_LIB"):
                L = pkg.lib()
                if hasattr(L, "gpsbb_test_despread_exact"):
                    L.gpsbb_test_despread_exact.argtypes = [C.c_void_p]
                    L.gpsbb_test_despread_exact.restype = C.c_ulonglong
                    exact += L.gpsbb_test_despread_exact(b._b)
                    print("%s: state granule log2 %d, the carrier's %d" % (name, L.gpsbb_test_state_log2(b._b),
                                                                          L.gpsbb_test_state_log2_carr(b._b)))
            b.close()
            if bad:
                print("%s (seed where %d):\n%s" % (name, where, "\n".join(bad)))
                return 1
            print("%s: pre-pass %d, %d views x 2 segment lengths x %d lags" % (name, s.info(pkg.INFO_PREPASS), len(views), len(LAGS)), flush=True)
    print("exact-path samples of the last despread of each batch: %d" % exact)
    print("despread at lags bit-exact against the oracle's replicas")
    return 0


if __name__ == "__main__":
    sys.exit(main())
