"""gpsbb_device_track against the numpy restatement (track_host over view_host): the cases and the comparison that
tests/test_track.py and tests/test_track_gpu.py share.  Every comparison is == on integers: every field of every record, every
count, every returned state.  Run as a script it checks the cases on the GPU and prints what it compared:

    python tools/track_check.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402

FS = ac.FS
NOISE = ac.NOISE
LEN = 1023 << 32
CODE_NOM_FAST = 3 << 31          # 1.5 chips per sample: N = 682 or 683, two full passes of 256 lanes and a ragged third
CARR_MAX = (1 << 47) - 1


def make_cfg(pkg, code_nom=CODE_NOM_FAST, nfll=6, max_epochs=12, gains=(157746, 42085, 842, 645, 0), spacing=1 << 31, aid_div=1540 << 16):
    """a configuration from its integers; gains = (kf, kp1, kp2, kd1, kd2), by default trk_make's at 2.6 MS/s"""
    c = pkg.TrkCfg()
    c.code_nom, c.aid_div, c.spacing, c.nfll, c.max_epochs = code_nom, aid_div, spacing, nfll, max_epochs
    c.kf, c.kp1, c.kp2, c.kd1, c.kd2 = gains
    return c


def make_states(pkg, rows):
    """TRK_STATE_DTYPE [len(rows)] from dicts of the fields that are not zero"""
    st = np.zeros(len(rows), pkg.TRK_STATE_DTYPE)
    for k, r in enumerate(rows):
        for f, v in r.items():
            st[k][f] = v
    return st


def step48(f_hz, fs=FS):
    """a carrier step in 2^-48 turns per sample"""
    return int(round(f_hz / fs * (1 << 48)))


def compare(got, want, what=""):
    """findings (strings) of (states, records per channel) against the same from the mirror, field by field"""
    bad = []
    (gs, gr), (ws, wr) = got, want
    if gs.shape != ws.shape or len(gr) != len(wr):
        return ["%s: %d states and %d record lists, want %d and %d" % (what, gs.size, len(gr), ws.size, len(wr))]
    for f in gs.dtype.names:
        if not (gs[f] == ws[f]).all():
            c = int(np.argwhere(gs[f] != ws[f])[0][0])
            bad.append("%s state.%s: channel %d has %d, want %d" % (what, f, c, gs[f][c], ws[f][c]))
    for c, (g, w) in enumerate(zip(gr, wr)):
        if g.shape != w.shape:
            bad.append("%s channel %d: %d records, want %d" % (what, c, g.size, w.size))
            continue
        for f in g.dtype.names:
            if not (g[f] == w[f]).all():
                k = int(np.argwhere(g[f] != w[f])[0][0])
                bad.append("%s channel %d record %d .%s: %d, want %d" % (what, c, k, f, g[f][k], w[f][k]))
    return bad


def on_device(pkg, synth, iq, cfg, states, view=0, noise=None, interf=None, nsamp=None):
    """the call on host array iq [n, 2] through a device buffer -> (states, records per channel)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(iq, np.int16)).cuda()
    torch.cuda.synchronize()
    return synth.device_track(t.data_ptr(), iq.shape[0] if nsamp is None else nsamp, cfg, states, view, noise, interf)


def mirror(pkg, iq, cfg, states, view=0, noise=None, interf=None, nsamp=None):
    n = iq.shape[0] if nsamp is None else nsamp
    return pkg.track_host(pkg.view_host(iq[:n], view, noise, interf=interf), cfg, states)


def check(pkg, synth, iq, cfg, states, view=0, noise=None, interf=None, nsamp=None, what=""):
    """findings of one call against the mirror fed with view_host's output of the first nsamp samples"""
    return compare(on_device(pkg, synth, iq, cfg, states, view, noise, interf, nsamp), mirror(pkg, iq, cfg, states, view, noise, interf, nsamp), what)


def records_cs(recs, state_after):
    """the code step each record's epoch ran with, from the code phases before and after it"""
    cp = [int(v) for v in recs["code_phase"]] + [int(state_after["code_phase"])]
    return [(cp[k + 1] - cp[k] + LEN) // int(recs["N"][k]) for k in range(recs.size)]


# ---- the cases ----

def lane_map_case(pkg):
    """random full-range IQ, N = 682 or 683, PRNs {1, 7, 17, 32} with different steps and code phases, nfll = 6, 12 epochs"""
    cfg = make_cfg(pkg, nfll=6, max_epochs=12)
    st = make_states(pkg, [dict(prn=1, carr_step=step48(1234.5), carr_int=step48(1234.5)),
                           dict(prn=7, n0=3, carr_step=step48(-4321.0), carr_int=step48(-4321.0), carr_phase=0x89ABCDEF, code_phase=(500 << 32) + 12345),
                           dict(prn=17, n0=700, carr_step=step48(250000.0), carr_int=step48(250000.0), carr_phase=0x7FFFFFFF, code_phase=LEN - 1),
                           dict(prn=32, n0=1, carr_step=-step48(640000.0), carr_int=-step48(640000.0), carr_phase=1, code_phase=1)])
    return ac.random_iq(700 + 13 * 683 + 40, 0xB1), cfg, st


def ends_case(pkg):
    """two channels on random IQ; the tests cut the buffer at the end of channel 0's fifth epoch"""
    cfg = make_cfg(pkg, nfll=2, max_epochs=64)
    st = make_states(pkg, [dict(prn=5, carr_step=step48(777.0), carr_int=step48(777.0), code_phase=(17 << 32) + 99),
                           dict(prn=9, n0=11, carr_step=step48(-1500.0), carr_int=step48(-1500.0))])
    return ac.random_iq(8 * 683, 0xB2), cfg, st


def views_case(pkg):
    """two channels, eight epochs, for every view and impairment"""
    cfg = make_cfg(pkg, nfll=4, max_epochs=8)
    st = make_states(pkg, [dict(prn=3, carr_step=step48(3210.0), carr_int=step48(3210.0), code_phase=(1000 << 32) + 7),
                           dict(prn=31, n0=5, carr_step=step48(-99999.0), carr_int=step48(-99999.0), carr_phase=0xDEADBEEF)])
    return ac.random_iq(9 * 683 + 20, 0xB3), cfg, st


def smallest_code_nom():
    """the smallest legal code_nom: ceil(LEN / (c - c // 8)) <= 2^20"""
    c = (LEN >> 20) * 8 // 7
    while -((-LEN) // (c - c // 8)) > 1 << 20:
        c += 1
    while -((-LEN) // ((c - 1) - (c - 1) // 8)) <= 1 << 20:
        c -= 1
    return c


def range_case(pkg):
    """every component -32768, carrier step 0 at table index 64 (45 degrees: |yI| at its largest), the smallest legal code_nom, all
    gains zero, two epochs of about 917000 samples"""
    nom = smallest_code_nom()
    cfg = make_cfg(pkg, code_nom=nom, nfll=1, max_epochs=2, gains=(0, 0, 0, 0, 0), aid_div=0)
    st = make_states(pkg, [dict(prn=13, carr_phase=64 << 23)])
    n = 2 * (-((-LEN) // nom)) + 3
    return np.full((n, 2), -32768, np.int16), cfg, st


def clamps_case(pkg):
    """kf, kp1 and kd1 at 2^31 - 1 on random data, 10 epochs, two channels that start near either end of the carrier's range"""
    big = (1 << 31) - 1
    cfg = make_cfg(pkg, nfll=5, max_epochs=10, gains=(big, big, 842, big, 0))
    near = CARR_MAX - (1 << 43)
    st = make_states(pkg, [dict(prn=2, carr_step=near, carr_int=near), dict(prn=30, carr_step=-near, carr_int=-near, code_phase=(77 << 32))])
    return ac.random_iq(11 * 800, 0xB50), cfg, st   # (a seed with which both ends of both clamps are reached: tests/test_track.py)


def resume_case(pkg):
    """40 epochs with noise; channels 0 and 1 are the same PRN in the same state"""
    cfg = make_cfg(pkg, nfll=20, max_epochs=40)
    same = dict(prn=11, n0=2, carr_step=step48(2222.0), carr_int=step48(2222.0), code_phase=(300 << 32) + 5)
    st = make_states(pkg, [same, same, dict(prn=24, carr_step=step48(-800.0), carr_int=step48(-800.0))])
    return ac.random_iq(41 * 683, 0xB6), cfg, st


# ---- end to end: six satellites rendered, acquired, tracked, their data bits read back ----

E2E_NSAMP = 1300000
E2E_ACQ_NSAMP = 7800
E2E_SKIP = 150
E2E_PRESENT = ac.E2E_PRESENT


def e2e_descriptors(pkg):
    return ac.e2e_descriptors(pkg)


def e2e_acq_cfg(pkg, view):
    return pkg.acq_make(1.0 / FS, -5000.0, 250.0, 41, 1e-3, 0, 2, view)


def e2e_trk_cfg(pkg):
    return pkg.trk_make(1.0 / FS)


def e2e_seeds(pkg, rows, acq_cfg):
    """one state per present PRN from its best cell"""
    st = np.zeros(len(E2E_PRESENT), pkg.TRK_STATE_DTYPE)
    for k, prn in enumerate(E2E_PRESENT):
        b, lag, _, _ = pkg.acq_best(rows, acq_cfg, prn)
        st[k] = pkg.trk_seed(acq_cfg, prn, b, lag)
    return st


def want_bits(d, first, n):
    """the n data bits (+-1) from record `first` on, as the descriptor d has them: epoch 0 is code period icode + 1 of bit (iword, ibit)"""
    g0 = int(d["iword"]) * 30 + int(d["ibit"]) + (int(d["icode"]) + 1 + first) // 20
    return np.array([((int(d["dwrd"][(g0 + b) // 30]) >> (29 - (g0 + b) % 30)) & 1) * 2 - 1 for b in range(n)], np.int8)


def e2e_findings(pkg, ch, recs, skip=E2E_SKIP):
    """(findings, figures) over the channels' records: per PRN the carrier within 1 Hz of f_carr over the last 50 epochs, one
    non-zero histogram bin, at (-(icode + 1)) mod 20, and the bits all equal or all opposite to the descriptor's; figures: the
    smallest |P.i| and the largest |P.q| after `skip`"""
    bad, min_pi, max_pq = [], None, 0
    for k, prn in enumerate(E2E_PRESENT):
        d, r = ch[0, prn - 1], recs[k]
        assert int(d["prn"]) == prn
        if r.size < skip + 60:
            bad.append("PRN %d: %d records" % (prn, r.size))
            continue
        f = float(np.mean(r["carr_step"][-50:].astype(np.float64))) / float(1 << 48) * FS
        if abs(f - float(d["f_carr"])) > 1.0:
            bad.append("PRN %d: carrier %.3f Hz, f_carr %.3f" % (prn, f, float(d["f_carr"])))
        off, hist = pkg.trk_bitsync(r, skip)
        if np.count_nonzero(hist) != 1:
            bad.append("PRN %d: histogram %s" % (prn, hist.tolist()))
        if off != (-(int(d["icode"]) + 1)) % 20:
            bad.append("PRN %d: offset %d, want %d" % (prn, off, (-(int(d["icode"]) + 1)) % 20))
        first = skip + ((off - skip) % 20)
        bits = pkg.trk_bits(r, first)
        want = want_bits(d, first, bits.size)
        if bits.size not in (16, 17) or not ((bits == want).all() or (bits == -want).all()):
            bad.append("PRN %d: %d bits %s, want +-%s" % (prn, bits.size, bits.tolist(), want.tolist()))
        pi, pq = np.abs(r["p_i"][skip:]), np.abs(r["p_q"][skip:])
        min_pi = int(pi.min()) if min_pi is None else min(min_pi, int(pi.min()))
        max_pq = max(max_pq, int(pq.max()))
    return bad, (min_pi, max_pq)


def main():
    sys.path.insert(0, ROOT)
    try:
        import torch  # noqa: F401  (one HIP runtime for torch and libgpsbb)
    except Exception:
        pass
    from __graft_entry__ import load_package
    pkg = load_package()
    bad = []
    with pkg.Synth(0) as s:
        iq, cfg, st = lane_map_case(pkg)
        bad += check(pkg, s, iq, cfg, st, what="lane map")
        print("lane map: 4 channels x 12 epochs", flush=True)
        for view in (pkg.OUT_SC16, pkg.OUT_SC8(5), pkg.OUT_SC1):
            iq, cfg, st = views_case(pkg)
            bad += check(pkg, s, iq, cfg, st, view, what="views 0x%x" % view)
            bad += check(pkg, s, iq, cfg, st, view, NOISE, what="views 0x%x noise" % view)
            print("view 0x%x: plain and with noise" % view, flush=True)
        iq, cfg, st = resume_case(pkg)
        bad += check(pkg, s, iq, cfg, st, 0, NOISE, what="40 epochs")
        print("40 epochs with noise", flush=True)
    if bad:
        print("\n".join(bad))
        return 1
    print("tracking bit-exact against the numpy mirror")
    return 0


if __name__ == "__main__":
    sys.exit(main())
