"""gpsbb_batch_despread against the numpy restatement (despread_host over view_host) fed with the CPU oracle's replicas.

The replica of channel i is the oracle's render of channel i ALONE at gain 1.0 with the same chaining (include/gpsbb.h: the
render is sum_i trunc(gain_i * r_i)).  This module is what tests/test_despread.py and tests/test_despread_gpu.py import for
that; run as a script it checks the four geometries below, chained, on one pre-pass and prints how many samples took the
kernel's exact path:

    python tools/despread_check.py [--where 0|1|2|3] [--views]
    GPSBB_PY_LIB=exp GPSBB_DS_DANGER=4194304 python tools/despread_check.py    (the exact path made common: the soak of the tests)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# GPSBB_VARIANT_* (include/gpsbb.h)
EV, EV_DENSE, PD_WIDE, PD_NARROW = 2, 3, 4, 5


def replicas(oracle, ch, delt, nsamp, chain=False):
    """r_i of every block, channel and sample: int16 [nblocks, nch, nsamp, 2] (c, s); zeros for idle channels"""
    ch = np.ascontiguousarray(ch)
    if ch.ndim == 1:
        ch = ch[None, :]
    nb, nch = ch.shape
    out = np.zeros((nb, nch, nsamp, 2), np.int16)
    for i in range(nch):
        if not (ch["prn"][:, i] > 0).any():
            continue
        one = ch.copy()
        one["prn"][:, np.arange(nch) != i] = 0
        one["gain"] = 1.0
        iq, _, _ = oracle.fill_blocks(one, delt, nsamp, chain=chain)
        out[:, i] = iq
    return out


def geometries(pkg):
    """name, fs, nsamp, descriptors [nblocks, nch], the kernel that renders them: the four model kernels' own ground, each with
    an idle channel, one that pauses for a block and a PRN hand-over; nsamp is a multiple neither of 1024 nor of 3 * 1024"""
    out = []
    for name, fs, nch, nsamp, nb, variant, seed in (("pd wide", 2.6e6, 12, 300000, 3, PD_WIDE, 11), ("pd narrow", 3e6, 16, 70001, 3, PD_NARROW, 12),
                                                    ("ev", 25e6, 16, 100001, 4, EV, 13), ("ev dense", 15.8565e6, 16, 70001, 3, EV_DENSE, 14)):
        ch = pkg.synth_descriptors(nb, nch=nch, seed=seed)
        if variant == EV_DENSE:   # one channel per breakpoint (a code slower than 1.023 Mchip/s), one per sample
            ch["f_carr"][:, 0], ch["f_carr"][:, 1] = -200.0, 3000.0
            ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
        ch["prn"][:, 3] = 0
        ch["prn"][1, 5] = 0
        ch["prn"][2:, 7] = 29
        out.append(dict(name=name, fs=fs, nsamp=nsamp, ch=ch, variant=variant))
    return out


def check_batch(pkg, synth, b, iq, rep, seg_tiles_list, views=((0, None),), d_iq=None):
    """findings (strings) of one run batch: its sums for every seg_tiles and (view, noise) against the host's"""
    bad = []
    for view, noise in views:
        u = pkg.view_host(iq, view, noise)
        for st in seg_tiles_list:
            got = b.despread(view=view, noise=noise, seg_tiles=st, d_iq=d_iq)
            want = pkg.despread_host(u, rep, st)
            if got.shape != want.shape or not (got == want).all():
                w = np.argwhere(got != want) if got.shape == want.shape else []
                bad.append("view 0x%x noise %s seg_tiles %d: %d sums differ, first (block, channel, segment, i/q) %s"
                           % (view, noise is not None, st, len(w), w[0].tolist() if len(w) else "shape"))
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
    nz = {"seed": 0xC0FFEE, "sample0": (1 << 33) + 12345, "sigma": 900.0, "shift": 1}
    views = [(pkg.OUT_SC16, None)]
    if "--views" in sys.argv:
        views += [(pkg.OUT_SC8(5), None), (pkg.OUT_SC1, None), (pkg.OUT_SC16, nz), (pkg.OUT_SC8(5), nz), (pkg.OUT_SC1, nz)]
    exact = 0
    with pkg.Synth(0) as s:
        s.set_option(pkg.OPT_SEED_WHERE, where)
        for g in geometries(pkg):
            delt = 1.0 / g["fs"]
            iq, _, _ = oracle.fill_blocks(g["ch"], delt, g["nsamp"], chain=True)
            rep = replicas(oracle, g["ch"], delt, g["nsamp"], chain=True)
            b = s.batch(g["ch"], delt, g["nsamp"], flags=pkg.CHAIN_CARRIER)
            b.run()
            s.sync()
            assert s.info(pkg.INFO_LAST_VARIANT) == g["variant"], (g["name"], s.info(pkg.INFO_LAST_VARIANT))
            ntiles = (g["nsamp"] + 1023) // 1024
            bad = check_batch(pkg, s, b, iq, rep, (1, 3, ntiles), views)
            if os.environ.get("GPSBB_PY_LIB"):
                L = pkg.lib()
                if hasattr(L, "gpsbb_test_despread_exact"):
                    L.gpsbb_test_despread_exact.argtypes = [C.c_void_p]
                    L.gpsbb_test_despread_exact.restype = C.c_ulonglong
                    exact += L.gpsbb_test_despread_exact(b._b)
                    print("%s: state granule log2 %d, the carrier's %d" % (g["name"], L.gpsbb_test_state_log2(b._b),
                                                                          L.gpsbb_test_state_log2_carr(b._b)))
            b.close()
            if bad:
                print("%s (seed where %d):\n%s" % (g["name"], where, "\n".join(bad)))
                return 1
            print("%s: pre-pass %d, %d views x 3 segment lengths" % (g["name"], s.info(pkg.INFO_PREPASS), len(views)), flush=True)
    print("exact-path samples of the last despread of each batch: %d" % exact)
    print("despread bit-exact against the oracle's replicas")
    return 0


if __name__ == "__main__":
    sys.exit(main())
