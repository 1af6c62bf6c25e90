"""The calls that read device IQ, one after the other on ONE handle: what no single-call test sees.  Their scratch is kept between
calls, so every call runs large, then small, then large again with the others in between: a stale partial sum, a row of the
larger search or a clip count that was not zeroed fails ==.  A second handle then makes one call of each kind and is closed, and the
first repeats its own: nothing is shared or freed across handles.  The cases are the check tools' (tools/*_check.py: the smallest
shapes at which each kernel can go wrong), the comparisons == against the numpy mirrors, computed once."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import acq_check as ac  # noqa: E402
import despread_check as dc  # noqa: E402
import fir_check as fc  # noqa: E402
import track_check as tc  # noqa: E402

LAGS = (-3, 0, 2)
DS_NOISE = {"seed": 0xC0FFEE, "sample0": (1 << 33) + 12345, "sigma": 900.0, "shift": 1}

_cases = {}


def cases(pkg, oracle):
    """every input and what its mirror makes of it, once per session (no GPU needed)"""
    if _cases:
        return _cases
    c = _cases
    # acquire: large with the grid, small without
    iq, cfg, n = ac.ragged_case(pkg)
    c["acq_big"] = dict(iq=iq[:n], cfg=cfg, want=pkg.acquire_host(pkg.view_host(iq[:n]), cfg),
                        want_nz=pkg.acquire_host(pkg.view_host(iq[:n], pkg.OUT_SC16, ac.NOISE), cfg))
    iq, cfg = ac.lane_map_case(pkg)
    c["acq_small"] = dict(iq=iq, cfg=cfg, want=pkg.acquire_host(pkg.view_host(iq), cfg))
    # track: 4 channels of 12 epochs, 2 channels
    for name, (iq, cfg, st) in (("trk_big", tc.lane_map_case(pkg)), ("trk_small", tc.ends_case(pkg))):
        c[name] = dict(iq=iq, cfg=cfg, st=st, want=tc.mirror(pkg, iq, cfg, st))
    # fir: the longest filter at the largest decimation over 4096 samples, at a shift with which some outputs clip; one tap over 4
    iq, fir = ac.random_iq(4096, 0xF129), fc.random_fir(pkg, 129, 16, 12, 0xF16)
    c["fir_big"] = dict(iq=iq, fir=fir, want=fc.mirror(pkg, iq, fir))
    assert c["fir_big"]["want"][2] > 0
    iq, fir = ac.random_iq(5, 0xF1)[:4], pkg.Fir([1], 1, 0)
    c["fir_small"] = dict(iq=iq, fir=fir, want=fc.mirror(pkg, iq, fir))
    # level, pack, digest: 3 blocks of 1024, and the first of them alone
    blocks = ac.random_iq(3 * 1024, 0x1E7).reshape(3, 1024, 2)
    c["blocks"] = dict(iq=blocks, sc8=pkg.OUT_SC8(5), level=pkg.level_host(blocks), level_nz=pkg.level_host(blocks, ac.NOISE),
                       pack8=pkg.pack_iq(blocks, pkg.OUT_SC8(5)), pack1=pkg.pack_iq(blocks, pkg.OUT_SC1), digest=pkg.block_digest_host(blocks))
    # despread: one small batch of tools/despread_check.py, its sums per tile (large), per block (small) and at lags
    g = [g for g in dc.geometries(pkg) if g["name"] == "pd narrow"][0]
    delt = 1.0 / g["fs"]
    iq = oracle.fill_blocks(g["ch"], delt, g["nsamp"], chain=True)[0]
    rep = dc.replicas(oracle, g["ch"], delt, g["nsamp"], chain=True)
    ntiles = (g["nsamp"] + 1023) // 1024
    c["ds"] = dict(g, delt=delt, ntiles=ntiles, big=pkg.despread_host(iq, rep, 1), small=pkg.despread_host(iq, rep, ntiles),
                   big_nz=pkg.despread_host(pkg.view_host(iq, pkg.OUT_SC16, DS_NOISE), rep, 1), lags=pkg.despread_lags_host(iq, rep, 3, LAGS))
    return c


class Calls:
    """one handle, its batch and the device copies of the cases' inputs; every method returns findings (strings)"""

    def __init__(self, pkg, c, dev):
        self.pkg, self.c, self.dev = pkg, c, dev
        self.s = pkg.Synth(0)
        self.b = None

    def close(self):
        if self.b is not None:
            self.b.close()
        self.s.close()

    def batch(self):
        g = self.c["ds"]
        self.b = self.s.batch(g["ch"], g["delt"], g["nsamp"], flags=self.pkg.CHAIN_CARRIER)
        self.b.run()
        self.s.sync()
        assert self.s.info(self.pkg.INFO_LAST_VARIANT) == g["variant"]

    def ptr(self, name):
        return self.dev[name].data_ptr()

    def acquire(self, name, grid, noise=None):
        k = self.c[name]
        want = k["want_nz" if noise else "want"]
        got = self.s.device_acquire(self.ptr(name), k["iq"].shape[0], k["cfg"], self.pkg.OUT_SC16, noise, None, want_grid=grid)
        return ac.compare(got[0], got[1], want[0], want[1], name) if grid else ac.compare(got, None, want[0], None, name)

    def track(self, name):
        k = self.c[name]
        return tc.compare(self.s.device_track(self.ptr(name), k["iq"].shape[0], k["cfg"], k["st"]), k["want"], name)

    def fir(self, name, cuts=()):
        """the call, or with cuts the same samples in pieces, each handed the history of the one before"""
        import torch
        k = self.c[name]
        D, n = int(k["fir"].decim), k["iq"].shape[0]
        out = torch.full((n // D + 3, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        hist, clips, at = None, 0, 0
        for end in tuple(cuts) + (n,):
            assert at % D == 0 and end % D == 0
            hist, cl = self.s.device_fir(self.ptr(name) + 4 * at, end - at, k["fir"], out.data_ptr() + 4 * (at // D), hist)
            clips, at = clips + cl, end
        got = out.cpu().numpy()
        assert (got[n // D:] == 0x5A5A).all(), "the call wrote behind its output"
        return fc.compare((got[:n // D], hist, clips), k["want"], "%s %s" % (name, list(cuts)))

    def blocks(self, nb, noise=None):
        """level, pack SC8, pack SC1 and both digests of the first nb blocks"""
        pkg, k, p = self.pkg, self.c["blocks"], self.ptr("blocks")
        bad = []
        lv = self.s.device_level(p, nb, 1024, noise)
        if lv.tobytes() != k["level_nz" if noise else "level"][:nb].tobytes():
            bad.append("level of %d blocks (noise %s)" % (nb, noise is not None))
        if not (self.s.device_pack(p, nb, 1024, k["sc8"]) == k["pack8"][:nb]).all():
            bad.append("pack SC8 of %d blocks" % nb)
        if not (self.s.device_pack(p, nb, 1024, pkg.OUT_SC1) == k["pack1"][:nb]).all():
            bad.append("pack SC1 of %d blocks" % nb)
        if not (self.s.device_digest(p, nb, 1024) == k["digest"][:nb]).all():
            bad.append("device_digest of %d blocks" % nb)
        if not (self.s.slot_digest(p, nb, 1024) == k["digest"][:nb]).all():
            bad.append("slot_digest of %d blocks" % nb)
        return bad

    def despread(self, which):
        g = self.c["ds"]
        if which == "lags":
            got = self.b.despread_lags(LAGS, seg_tiles=3)
        else:
            got = self.b.despread(noise=DS_NOISE if which == "big_nz" else None, seg_tiles=g["ntiles"] if which == "small" else 1)
        want = g[which]
        return [] if got.shape == want.shape and (got == want).all() else ["despread %s: %s sums differ" % (
            which, int((got != want).sum()) if got.shape == want.shape else "shape")]


@pytest.mark.gpu
def test_scratch_across_calls_and_handles(pkg, oracle):
    import torch
    c = cases(pkg, oracle)
    dev = {name: torch.from_numpy(np.ascontiguousarray(k["iq"], np.int16)).cuda() for name, k in c.items() if name != "ds"}
    torch.cuda.synchronize()
    a = Calls(pkg, c, dev)
    bad = []
    try:
        bad += a.blocks(3, ac.NOISE)          # a fresh handle's first call has noise: the knot table is made by the prologue
        a.batch()
        # large
        bad += a.acquire("acq_big", True) + a.despread("big") + a.track("trk_big") + a.fir("fir_big") + a.blocks(3) + a.despread("lags")
        # small: every buffer is reused below its size
        bad += a.acquire("acq_small", False) + a.track("trk_small") + a.despread("small") + a.fir("fir_small") + a.blocks(1)
        # large again, in another order, with a late call with noise of either kind
        bad += a.fir("fir_big", cuts=(2048,)) + a.blocks(3) + a.acquire("acq_big", True) + a.despread("big_nz") + a.track("trk_big")
        bad += a.acquire("acq_big", True, ac.NOISE) + a.despread("lags") + a.despread("big")
        # a second handle makes one call of each kind and goes
        b = Calls(pkg, c, dev)
        try:
            b.batch()
            bad += ["second handle: " + f for f in b.blocks(1) + b.acquire("acq_small", True) + b.track("trk_small") + b.fir("fir_small")
                    + b.despread("small") + b.despread("lags")]
        finally:
            b.close()
        # ... and the first goes on as if nothing had happened
        bad += a.blocks(3) + a.acquire("acq_big", True) + a.track("trk_big") + a.fir("fir_big") + a.despread("big") + a.despread("lags")
    finally:
        a.close()
    assert not bad, "\n".join(bad)
