"""The corner table of the descriptor contract (include/gpsbb.h): code rates on either side of every threshold ev_plan()
decides on, gains at the model kernels' admission limit and at the contract's edge, peaks two counts from where the packed
I/Q arithmetic stops being exact, every PRN.  Built once, deterministically, for tests/test_contract_corners.py (CPU: the
oracle against the reference's own loop), tests/test_contract_corners_gpu.py (every kernel against the oracle) and
tests/golden/make_golden.py (the fixture that pins the GPU machine to the reference).  A plain helper, not a conftest.

Every case carries the synthesis kernel it must be rendered by when the library chooses (`variant`), written out below from
the documented rules, not asked of the library:

  * a block goes to k_synth when any active channel has f_code*delt < 2^-20 or > 543/1040 (1023 + 1040*sc + 2 <= 1568), or
    when sum(512*|gain| + 1) over its active channels reaches 32768;
  * a channel is evaluated per sample when sc*15.5 >= 1 (more than one chip change per run of 16 samples) or when its carrier
    changes the table index more than four times per run (|f_carr*delt|*512*15.5 >= 4); a carrier slower than 2^-27 index
    units per sample is always recomputed exactly and never counts as per-sample;
  * no channel per sample: k_synth_ev; some: k_synth_ev_dense; all: k_synth_pd, wide up to 12 channel SLOTS, narrow above;
  * GPSBB_FIXED_CARRIER: k_synth_ev_fixed when no channel is per sample, k_synth_pd when all are (per-sample code and an
    index step below 64), k_synth otherwise: there is no mixed kernel for the accumulator.

So that these hold whatever the other Dopplers are, channel 0 of every drawn block has a Doppler in (-400, 0) Hz (at most
four index changes per run down to 1 MS/s, and a code slower than 1.023 Mchip/s: per breakpoint at 15.8565 MS/s) and channel 1
one in (2000, 5000) Hz (per sample at 2.6 and 1 MS/s, and at 15.8565 MS/s through its faster code)."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob

CHAN = ob.CHAN_DTYPE
NSAMP_CODE, NSAMP_GAIN = 70001, 30001
RATES_CODE = (25e6, 16.368e6, 2.6e6, 1e6)
RATES_GAIN = (25e6, 15.8565e6, 2.6e6, 1e6)
RATES_PEAK = (25e6, 15.8565e6, 2.6e6)
SLOTS = (12, 16)

# GPSBB_VARIANT_* (include/gpsbb.h)
SYNTH, EV, EV_DENSE, PD_WIDE, PD_NARROW, EV_FIXED = 1, 2, 3, 4, 5, 6
VARIANT_NAMES = {SYNTH: "k_synth", EV: "k_synth_ev", EV_DENSE: "k_synth_ev_dense", PD_WIDE: "k_synth_pd wide",
                 PD_NARROW: "k_synth_pd narrow", EV_FIXED: "k_synth_ev_fixed"}
MODEL_VARIANTS = (EV, EV_DENSE, PD_WIDE, PD_NARROW, EV_FIXED)

# the products f_code*delt, in the order of the contract
SC = {
    "below 2^-20": math.nextafter(2.0 ** -20, 0.0),
    "2^-20": 2.0 ** -20,
    "1e-4": 1e-4,
    "1/15.5-": math.nextafter(1 / 15.5, 0.0),
    "1/15.5+": math.nextafter(math.nextafter(1 / 15.5, 1.0), 1.0),
    "0.25": 0.25,
    "0.5": 0.5,
    "542/1040-": math.nextafter(542.0 / 1040.0, 0.0),
    "542.5/1040": 542.5 / 1040.0,
    "543/1040-": 543.0 / 1040.0 - 2.0 ** -45,   # the last product ev_plan admits
    "543/1040+": 543.0 / 1040.0 + 2.0 ** -45,   # the first it declines
    "1-": 1.0 - 2.0 ** -30,
    "1": 1.0,
    "1+": 1.0 + 2.0 ** -30,
    "1.25": 1.25,
    "1.5": 1.5,
}
REACH = ("542/1040-", "542.5/1040", "543/1040-", "543/1040+")   # the chip table's reach: code phases aimed at 1023-
MIXED = ("2^-20", "1e-4", "1/15.5-", "1/15.5+", "0.25", "0.5", "543/1040-")

# ---- the variant column --------------------------------------------------------------------------------------------------
# "pd" reads k_synth_pd wide for 12 slots, narrow for 16.
_SLOW, _FAST, _OUT = ("2^-20", "1e-4", "1/15.5-"), ("1/15.5+", "0.25", "0.5", "542/1040-", "542.5/1040", "543/1040-"), \
    ("below 2^-20", "543/1040+", "1-", "1", "1+", "1.25", "1.5")


def _column(slow, fast, out="synth"):
    d = {n: slow for n in _SLOW}
    d.update({n: fast for n in _FAST})
    d.update({n: out for n in _OUT})
    return d


CODE_RATE_VARIANT = {   # every channel at one product
    25e6: _column("ev", "pd"), 16.368e6: _column("ev", "pd"),
    2.6e6: _column("dense", "pd"), 1e6: _column("dense", "pd"),      # channel 1's carrier is per sample there
}
CODE_RATE_VARIANT_FIXED = {
    25e6: _column("ev_fixed", "pd"),
    2.6e6: _column("synth", "pd"),                                    # channel 1: more than four index changes per run
}
# gains and peaks are drawn at the physical code rate, sc = (1.023e6 + f_carr/1540) / fs: 0.041 at 25 MS/s; on either side of
# 1/15.5 at 15.8565 MS/s = 15.5 * 1.023e6 (channel 0 below, channel 1 above); 0.39 at 2.6 MS/s; 1.023 at 1 MS/s: k_synth
MODEL_AT = {25e6: "ev", 15.8565e6: "dense", 2.6e6: "pd", 1e6: "synth"}
MODEL_AT_FIXED = {25e6: "ev_fixed", 15.8565e6: "synth", 2.6e6: "pd", 1e6: "synth"}
GAIN_UNDER = {"negative": True, "alternating": True, "tiny": True, "one large": True, "sum just under": True,
              "sum just under, negative": True, "sum just over": False, "sum just over, negative": False,
              "wraps int16": False, "contract edge": False}
# P1 / P3: one channel, Doppler +4000 Hz * fs/25e6, so its code is faster than 1.023 Mchip/s: per sample at 15.8565 MS/s, and
# then every active channel is; P2: zero-Doppler carriers (never per sample by themselves) on the drawn code rates
PEAK_VARIANT = {"P1": {25e6: "ev", 15.8565e6: "pd", 2.6e6: "pd"}, "P2": {25e6: "ev", 15.8565e6: "dense", 2.6e6: "pd"},
                "P3": {25e6: "synth", 15.8565e6: "synth", 2.6e6: "synth"}}
PEAK_VARIANT_FIXED = {"P1": {25e6: "ev_fixed", 15.8565e6: "pd", 2.6e6: "pd"},
                      "P2": {25e6: "ev_fixed", 15.8565e6: "synth", 2.6e6: "pd"},
                      "P3": {25e6: "synth", 15.8565e6: "synth", 2.6e6: "synth"}}
# mixed code rates in one block, and per-sample code beside carriers of every class (one of them always recomputed exactly:
# it keeps that class, so not every channel is per sample).  The accumulator has no such class: all per sample there.
MIXED_VARIANT, MIXED_VARIANT_FIXED = "dense", "synth"
CLASSES_VARIANT, CLASSES_VARIANT_FIXED = "dense", "pd"


def _variant(word, nch):
    return {"synth": SYNTH, "ev": EV, "dense": EV_DENSE, "ev_fixed": EV_FIXED, "pd": PD_WIDE if nch <= 12 else PD_NARROW}[word]


# ---- descriptors ---------------------------------------------------------------------------------------------------------

DWRD_POOLS = 8
_pool = None


def dwrd_pool():
    """the nav words: eight sets of 16 x 60 random 30-bit words, one of them per case (the fixture stores the sets once)"""
    global _pool
    if _pool is None:
        _pool = np.random.default_rng(0xD3AD).integers(0, 1 << 30, (DWRD_POOLS, 16, 60)).astype(np.uint32)
    return _pool


def base(nch, seed, prn0=1):
    rng = np.random.default_rng(seed)
    ch = np.zeros(nch, CHAN)
    ch["prn"] = (np.arange(nch) + prn0 - 1) % 32 + 1
    ch["f_carr"] = rng.uniform(-5000, 5000, nch)
    ch["f_carr"][0] = -rng.uniform(1.0, 400.0)
    ch["f_carr"][1] = rng.uniform(2000.0, 5000.0)
    ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540
    ch["code_phase"] = rng.uniform(0, 1023, nch)
    ch["carr_phase"] = rng.uniform(0, 1, nch)
    ch["gain"] = rng.uniform(0.3, 0.8, nch)
    ch["iword"] = rng.integers(0, 59, nch)
    ch["ibit"] = rng.integers(0, 30, nch)
    ch["icode"] = rng.integers(0, 20, nch)
    ch["dwrd"] = dwrd_pool()[seed % DWRD_POOLS, :nch]
    return ch


def f_code_for(sc, fs):
    """an f_code whose individually rounded product with delt = 1/fs is exactly sc (searched among the doubles next to sc*fs)"""
    delt = 1.0 / fs
    f = sc * fs
    for _ in range(200):
        p = f * delt
        if p == sc:
            return f
        f = math.nextafter(f, math.inf if p < sc else -math.inf)
    raise AssertionError("no f_code gives f_code*delt == %r at %g S/s" % (sc, fs))


def aim_code_below_1023(pkg, x0, s, n):
    """a code phase from which the reference's recurrence (c:2709-2737, the exact jump-ahead of the experiments build's host
    hooks) stands within 2^-10 chips below 1023 after n steps of s"""
    L = pkg.exp_lib()
    wr = C.c_longlong(0)
    want = 1023.0 - 2.0 ** -11
    x = x0
    for _ in range(8):
        got = L.gpsbb_test_code_jump(x, s, n, C.byref(wr))
        err = got - want
        if err < -511.5:
            err += 1023.0
        if -2.0 ** -11 < err < 2.0 ** -11:
            return x
        x = (x - err) % 1023.0
    raise AssertionError("could not aim the code NCO at 1023- (sc %r, sample %d)" % (s, n))


def fixed_of(ch):
    """the same block for GPSBB_FIXED_CARRIER: carr_phase as the 32-bit accumulator's value"""
    c = ch.copy()
    c["carr_phase"] = np.floor(c["carr_phase"] * 2.0 ** 32)
    return c


GAINS = {
    "negative": lambda n: -np.linspace(0.3, 0.8, n),
    "alternating": lambda n: np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * np.linspace(0.05, 1.5, n),
    "tiny": lambda n: np.array([0.0, -0.0, 5e-324, 1e-3, 0.0039, 0.004, 0.0041, -0.004] * 2)[:n],
    "one large": lambda n: np.r_[63.0, np.full(n - 1, 0.01)],
    "sum just under": lambda n: np.full(n, (32768.0 - n) / 512.0 / n * (1 - 2.0 ** -40)),
    "sum just over": lambda n: np.full(n, (32768.0 - n) / 512.0 / n * (1 + 2.0 ** -40)),
    "sum just under, negative": lambda n: -np.full(n, (32768.0 - n) / 512.0 / n * (1 - 2.0 ** -40)),
    "sum just over, negative": lambda n: -np.full(n, (32768.0 - n) / 512.0 / n * (1 + 2.0 ** -40)),
    "wraps int16": lambda n: np.full(n, 40.0),
    "contract edge": lambda n: np.r_[2097151.5, -2097151.5, np.full(n - 2, 0.5)],
}


def carrier_classes(fs, nch):
    """Dopplers of every class the planner tells apart: zero, always recomputed (|f_carr*delt*512| < 2^-27), ordinary of both
    signs, more than four index changes per run, the contract's fast end"""
    cls = [0.0, 2.0 ** -29 / 512 * fs, -2.0 ** -29 / 512 * fs, 1200.0 * fs / 25e6, -4999.0 * fs / 25e6,
           0.3 / 15.5 / 512 * fs * 16, -0.05 * fs]
    return [cls[i % len(cls)] for i in range(nch)]


_TABLE = None


def table(pkg):
    """the list of cases: dicts of name, kind, fs, nsamp, ch (CHAN[nch]), fixed, variant, base (the index of the IEEE case a
    fixed one was made from, or -1), peak (None, or (which, carr_phase) of a peak case), sc (the common product, or None)"""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    cases = []
    n = [0]

    def add(name, kind, fs, nsamp, ch, word, word_fixed=None, peak=None, sc=None, ch_fixed=None):
        cases.append(dict(name=name, kind=kind, fs=fs, nsamp=nsamp, ch=ch, fixed=False, variant=_variant(word, len(ch)), base=-1,
                          peak=peak, sc=sc))
        if word_fixed is not None:
            cases.append(dict(name=name + " fixed", kind=kind, fs=fs, nsamp=nsamp, ch=fixed_of(ch) if ch_fixed is None else ch_fixed, fixed=True,
                              variant=_variant(word_fixed, len(ch)), base=len(cases) - 1, peak=peak, sc=sc))

    def fresh(nch):
        n[0] += 1
        return base(nch, 1000 + n[0], prn0=1 + (n[0] * 5) % 32)

    for fs in RATES_CODE:
        for name, sc in SC.items():
            for nch in SLOTS:
                ch = fresh(nch)
                ch["f_code"] = f_code_for(sc, fs)
                if name in REACH:
                    ch["code_phase"][0] = math.nextafter(1023.0, 0.0)
                    for i, tile in ((2, 3), (5, 41)):
                        ch["code_phase"][i] = aim_code_below_1023(pkg, float(ch["code_phase"][i]), sc, 1024 * tile)
                fx = CODE_RATE_VARIANT_FIXED.get(fs)
                add("code %s %g %d" % (name, fs, nch), "code", fs, NSAMP_CODE, ch, CODE_RATE_VARIANT[fs][name],
                    fx[name] if fx else None, sc=sc)
    for fs in RATES_CODE:
        for nch in SLOTS:
            ch = fresh(nch)
            for i in range(nch):
                ch["f_code"][i] = f_code_for(SC[MIXED[i % len(MIXED)]], fs)
            add("mixed code rates %g %d" % (fs, nch), "mixed", fs, NSAMP_CODE, ch, MIXED_VARIANT, MIXED_VARIANT_FIXED)
            ch = fresh(nch)
            ch["f_code"] = f_code_for(0.25, fs)
            ch["f_carr"] = carrier_classes(fs, nch)
            add("carrier classes %g %d" % (fs, nch), "mixed", fs, NSAMP_CODE, ch, CLASSES_VARIANT, CLASSES_VARIANT_FIXED, sc=0.25)
    for fs in RATES_GAIN:
        for name, g in GAINS.items():
            for nch in SLOTS:
                ch = fresh(nch)
                ch["gain"] = g(nch)
                under = GAIN_UNDER[name]
                add("gain %s %g %d" % (name, fs, nch), "gain", fs, NSAMP_GAIN, ch, MODEL_AT[fs] if under else "synth",
                    MODEL_AT_FIXED[fs] if under else "synth")
    for fs in RATES_PEAK:
        for nch in SLOTS:
            for which, gain in (("P1", math.nextafter(32767 / 512, 0.0)), ("P3", 100.0)):
                ch = fresh(nch)
                ch["prn"][1:] = 0
                ch["gain"][0] = gain
                ch["f_carr"][0] = 4000.0 * fs / 25e6
                ch["f_code"][0] = 1.023e6 + ch["f_carr"][0] / 1540
                add("peak %s %g %d" % (which, fs, nch), "peak", fs, NSAMP_CODE, ch, PEAK_VARIANT[which][fs],
                    PEAK_VARIANT_FIXED[which][fs], peak=(which, None))
            for cp in (0.0, 0.25, 0.5, 0.75):
                ch = fresh(nch)
                ch["gain"] = 0.0
                ch["gain"][:3] = (32768.0 - nch) / 1536.0 * (1 - 2.0 ** -40)
                ch["f_carr"] = 0.0
                ch["carr_phase"] = cp
                # (the accumulator counts 2^-16 table-index units, 2^25 to the cycle: floor(cp * 2^32) would put all four phases
                # on index 0, so this one is initialised as allocateChannel does, c:1966-1967, and selects the same quadrants)
                chf = ch.copy()
                chf["carr_phase"] = math.floor(512 * 65536 * cp)
                add("peak P2 %g %g %d" % (cp, fs, nch), "peak", fs, NSAMP_CODE, ch, PEAK_VARIANT["P2"][fs],
                    PEAK_VARIANT_FIXED["P2"][fs], peak=("P2", cp), ch_fixed=chf)
    _TABLE = cases
    return cases


def redrawn_chain(case, nblocks=3):
    """the case as `nblocks` consecutive blocks (GPSBB_CHAIN_CARRIER) with the code phases of the later blocks redrawn"""
    rng = np.random.default_rng(len(case["name"]) * 7919 + int(case["fs"]) % 1009)
    ch = np.stack([case["ch"]] * nblocks)
    ch["code_phase"][1:] = rng.uniform(0, 1023, ch["code_phase"][1:].shape)
    return ch


# ---- the fixture (tests/golden/contract_corners.npz) ------------------------------------------------------------------------
# per case: fs, nsamp, slots, fixed, the descriptors, SHA-256 of the reference loop's IQ, its end states.  Descriptors and end
# states are stored for 16 slots (zeros beyond the case's own); the descriptors without their nav words, which are one of the
# eight sets of `dwrd_pool` (stored once), and only for the IEEE cases: a fixed case is fixed_of() its `base`.

SCALARS = np.dtype([(n, CHAN.fields[n][0]) for n in CHAN.names if n != "dwrd"])


def fixture_arrays(cases, iq_sha, end_states):
    nc = len(cases)
    own = [k for k, c in enumerate(cases) if c["base"] < 0]
    row = {k: r for r, k in enumerate(own)}
    desc = np.zeros((len(own), 16), SCALARS)
    pool_of = np.zeros(len(own), np.int32)
    st = np.zeros((nc, 16), ob.STATE_DTYPE)
    for k, c in enumerate(cases):
        st[k, :len(c["ch"])] = end_states[k]
        if c["base"] < 0:
            for f in SCALARS.names:
                desc[f][row[k], :len(c["ch"])] = c["ch"][f]
            match = [p for p in range(DWRD_POOLS) if (dwrd_pool()[p, :len(c["ch"])] == c["ch"]["dwrd"]).all()]
            pool_of[row[k]] = match[0]
    return dict(names=np.array([c["name"] for c in cases]), fs=np.array([c["fs"] for c in cases]),
                nsamp=np.array([c["nsamp"] for c in cases], np.int32), nch=np.array([len(c["ch"]) for c in cases], np.int32),
                fixed=np.array([c["fixed"] for c in cases]), variant=np.array([c["variant"] for c in cases], np.int32),
                desc_row=np.array([row[k] if c["base"] < 0 else row[c["base"]] for k, c in enumerate(cases)], np.int32),
                desc=desc.view(np.uint8).reshape(len(own), -1), dwrd_pool=dwrd_pool(), dwrd_of=pool_of,
                end_state=st.view(np.uint8).reshape(nc, -1), iq_sha256=np.array(iq_sha))


def fixture_descriptors(z, k):
    """case k's descriptors (CHAN[nch]) as the fixture `z` (the loaded .npz) holds them"""
    r, nch = int(z["desc_row"][k]), int(z["nch"][k])
    sc = z["desc"][r].view(SCALARS)[:nch]
    ch = np.zeros(nch, CHAN)
    for f in SCALARS.names:
        ch[f] = sc[f]
    ch["dwrd"] = z["dwrd_pool"][int(z["dwrd_of"][r]), :nch]
    if not bool(z["fixed"][k]):
        return ch
    if str(z["names"][k]).startswith("peak P2"):
        ch["carr_phase"] = np.floor(512 * 65536 * ch["carr_phase"])
        return ch
    return fixed_of(ch)
