"""pluto-gps-sim_amd — MI355X-native GPS L1 C/A baseband IQ synthesis (libgpsbb) for Python callers.

This is only a ctypes veneer over the C ABI in include/gpsbb.h: the product is libgpsbb.so
(hand-written HIP for gfx950 in csrc/).  There is no Python or CPU implementation of the fill here; every
fill call goes through the shared library and raises when the library or a GPU is missing.

The directory name contains '-' (it mirrors the reference's repo name), so import it by path:

    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("pluto_gps_sim_amd", ".../pluto-gps-sim_amd/__init__.py")
    mod = importlib.util.module_from_spec(spec); sys.modules[spec.name] = mod; spec.loader.exec_module(mod)

(`__graft_entry__.load_package()` and tests/conftest.py do exactly that.)
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# The product is libgpsbb.so: it reads no environment variable and exports include/gpsbb.h and one counter of what it holds
# (gpsbb_test_live), nothing else.  The experiments build of the same sources (libgpsbb_exp.so: measurement knobs from the
# environment, gpsbb_test_* hooks) is what the tuning scripts under tools/ use when they say so (GPSBB_PY_LIB=exp, read HERE, in
# the Python veneer) and what exp_lib() hands to the NCO unit tests.
_which = os.environ.get("GPSBB_PY_LIB")  # "exp", the tag of a variant a tuning script built (libgpsbb_<tag>.so), or the PATH of a library
# (the deliberately wrong builds of the tests live in the tests' temporary directories, never beside the product)
LIB_PATH = _which if _which and os.sep in _which else os.path.join(HERE, "libgpsbb_%s.so" % _which if _which else "libgpsbb.so")
EXP_LIB_PATH = os.path.join(HERE, "libgpsbb_exp.so")

MAX_CHAN = 16
N_DWRD = 60

CHAN_DTYPE = np.dtype([("prn", "<i4"), ("iword", "<i4"), ("ibit", "<i4"), ("icode", "<i4"),
                       ("f_carr", "<f8"), ("f_code", "<f8"), ("carr_phase", "<f8"),
                       ("code_phase", "<f8"), ("gain", "<f8"), ("dwrd", "<u4", (N_DWRD,))])
STATE_DTYPE = np.dtype([("carr_phase", "<f8"), ("code_phase", "<f8"), ("iword", "<i4"),
                        ("ibit", "<i4"), ("icode", "<i4"), ("dataBit", "<i4"), ("codeCA", "<i4"),
                        ("_pad", "<i4")])
# The reference's channel_t (plutogpssim.h:152-174, FLOAT_CARR_PHASE build, LP64) as a numpy record: what a caller that kept the
# reference's structures hands to gpsbb_fill_block_ref.  tests/test_ref_layout.py checks every offset against offsetof() on the
# real header (in the build container, where /root/reference exists).
REF_CHANNEL_DTYPE = np.dtype([("prn", "<i4"), ("ca", "<i4", (1023,)), ("f_carr", "<f8"), ("f_code", "<f8"),
                              ("carr_phase", "<f8"), ("code_phase", "<f8"), ("g0_week", "<i4"), ("_p0", "<i4"),
                              ("g0_sec", "<f8"), ("sbf", "<u8", (50,)), ("dwrd", "<u8", (60,)), ("iword", "<i4"),
                              ("ibit", "<i4"), ("icode", "<i4"), ("dataBit", "<i4"), ("codeCA", "<i4"), ("_p1", "<i4"),
                              ("azel", "<f8", (2,)), ("rho0", "<f8", (8,))])
# ... and the same struct of a reference built WITHOUT FLOAT_CARR_PHASE (h:12 removed): h:160-161 put a 32-bit accumulator and its
# step where the double was (same size, so nothing else moves): what gpsbb_fill_block_ref_fixed is handed
REF_CHANNEL_FIXED_DTYPE = np.dtype([("prn", "<i4"), ("ca", "<i4", (1023,)), ("f_carr", "<f8"), ("f_code", "<f8"),
                                    ("carr_phase", "<u4"), ("carr_phasestep", "<i4"), ("code_phase", "<f8"), ("g0_week", "<i4"),
                                    ("_p0", "<i4"), ("g0_sec", "<f8"), ("sbf", "<u8", (50,)), ("dwrd", "<u8", (60,)),
                                    ("iword", "<i4"), ("ibit", "<i4"), ("icode", "<i4"), ("dataBit", "<i4"), ("codeCA", "<i4"),
                                    ("_p1", "<i4"), ("azel", "<f8", (2,)), ("rho0", "<f8", (8,))])


class RefLayout(C.Structure):
    """gpsbb_ref_layout_t (include/gpsbb.h): where the fields gpsbb_fill_block_ref reads and updates sit in the caller's channel_t"""
    _fields_ = [(n, C.c_size_t) for n in ("stride", "off_prn", "off_f_carr", "off_f_code", "off_carr_phase", "off_code_phase",
                                          "off_dwrd", "sizeof_dwrd_elem", "off_iword", "off_ibit", "off_icode", "off_dataBit",
                                          "off_codeCA")]


def ref_layout(dtype=None):
    dtype = REF_CHANNEL_DTYPE if dtype is None else dtype
    off = lambda n: dtype.fields[n][1]
    return RefLayout(dtype.itemsize, off("prn"), off("f_carr"), off("f_code"), off("carr_phase"), off("code_phase"), off("dwrd"), 8,
                     off("iword"), off("ibit"), off("icode"), off("dataBit"), off("codeCA"))


def ref_channels(d):
    """one block's descriptors (CHAN_DTYPE[nch]) as the reference's channel_t[] and gain[] (plutogpssim.c:2241)"""
    chan = np.zeros(d.shape[0], REF_CHANNEL_DTYPE)
    for f in ("prn", "f_carr", "f_code", "carr_phase", "code_phase", "iword", "ibit", "icode"):
        chan[f] = d[f]
    chan["dwrd"] = d["dwrd"]
    return chan, np.ascontiguousarray(d["gain"])


ROW_DTYPE = np.dtype([("n0", "<i4"), ("nav", "<u4"), ("xb", "<u8"), ("inc", "<i8")])
assert CHAN_DTYPE.itemsize == 296 and STATE_DTYPE.itemsize == 40 and ROW_DTYPE.itemsize == 24

CHAIN_CARRIER = 1
FIXED_CARRIER = 2
STREAM_DEVICE_ONLY = 4
OPT_SEED_WHERE, OPT_SYNTH_KERNEL, OPT_SKIP_SEED, OPT_CHAIN_WHERE = 1, 2, 3, 4
INFO_LAST_KERNEL, INFO_EXACT_RUNS, INFO_CHAIN_ON_DEVICE, INFO_CHAIN_FALLBACKS, INFO_CHAIN_TIES, INFO_CHAIN_REPAIRS = 1, 2, 3, 4, 5, 6
INFO_STREAMS, INFO_HW_QUEUES, INFO_TILES_RENDERED, INFO_PREPASS = 7, 8, 9, 10
NODE_INDEXED, NODE_CONCURRENT, NODE_DEVICE_ONLY, NODE_NO_AFFINITY, NODE_FIXED_CARRIER, NODE_INTERLEAVED, NODE_DIGESTS = 1, 2, 4, 8, 16, 32, 64
PUSH_NEW_CHAIN = 1
PUSH_DIGEST = 2
PUSH_LEVEL = 4
NODE_MAX_SHARDS = 64
INFO_SC8_CLIPPED = 11
INFO_LAST_VARIANT = 13  # GPSBB_VARIANT_*: which synthesis kernel exactly
VARIANT_SYNTH, VARIANT_EV, VARIANT_EV_DENSE, VARIANT_PD_WIDE, VARIANT_PD_NARROW, VARIANT_EV_FIXED = 1, 2, 3, 4, 5, 6
# output formats of the host-bound paths (include/gpsbb.h GPSBB_OUT_*): the `fmt=` of fill_block / stream / Node / device_pack
OUT_SC16 = 0
OUT_SC1 = 2 << 8
OUT_FORMAT_MASK, OUT_SHIFT_MASK = 0xF00, 0xF000


def OUT_SC8(shift):
    """GPSBB_OUT_SC8(shift): int8 I/Q, clamp(v >> shift, -128, 127)"""
    return (1 << 8) | (int(shift) << 12)


# receiver noise on the host-bound outputs (include/gpsbb.h gpsbb_noise_t): the `noise=` of fill_block / stream / Node
INFO_NOISE_CLIPPED = 12
NOISE_KNOTS = 1665


class Noise(C.Structure):
    """gpsbb_noise_t: seed (the Philox key), sample0 (stream position of the first sample), sigma (per component, int16 LSB),
    shift (0..7: w = sat16((v + N) >> shift))"""
    _fields_ = [("seed", C.c_uint64), ("sample0", C.c_uint64), ("sigma", C.c_double), ("shift", C.c_int32), ("_pad", C.c_int32)]


def _as_noise(noise):
    """None, a Noise, or a dict with seed / sigma and optionally sample0 / shift -> a Noise (or None)"""
    if noise is None or isinstance(noise, Noise):
        return noise
    d = dict(noise)
    return Noise(int(d["seed"]) & 0xFFFFFFFFFFFFFFFF, int(d.get("sample0", 0)), float(d["sigma"]), int(d.get("shift", 0)), 0)


# interference on the host-bound outputs (include/gpsbb.h gpsbb_interf_t): the `interf=` of fill_block / stream / Node / despread
INTERF_CW, INTERF_CHIRP, INTERF_MAX = 0, 1, 4


class Interf(C.Structure):
    """gpsbb_interf_t: one emitter (interf_make builds it from physical units)"""
    _fields_ = [("kind", C.c_int32), ("level_q16", C.c_uint32), ("phase0", C.c_uint64), ("step", C.c_int64), ("rate", C.c_int64),
                ("sweep", C.c_uint32), ("pulse_period", C.c_uint32), ("pulse_on", C.c_uint32), ("pulse_offset", C.c_uint32)]


class InterfSet(C.Structure):
    """gpsbb_interf_set_t: n emitters, the shift of step 4, the stream position of the first sample"""
    _fields_ = [("n", C.c_int32), ("shift", C.c_int32), ("sample0", C.c_uint64), ("e", Interf * INTERF_MAX)]

    def __init__(self, emitters=(), shift=0, sample0=0):
        super().__init__()
        emitters = list(emitters)
        if len(emitters) > INTERF_MAX:
            raise ValueError("at most %d emitters" % INTERF_MAX)
        self.n, self.shift, self.sample0 = len(emitters), int(shift), int(sample0)
        for k, e in enumerate(emitters):
            self.e[k] = e


def _as_interf(interf):
    """None, an InterfSet, or a dict with emitters and optionally shift / sample0 -> an InterfSet (or None)"""
    if interf is None or isinstance(interf, InterfSet):
        return interf
    d = dict(interf)
    return InterfSet(d.get("emitters", ()), d.get("shift", 0), d.get("sample0", 0))


def _ref(x):
    return None if x is None else C.byref(x)


# output level (include/gpsbb.h gpsbb_level_t): one record per block, what device_level / Stream.pop_level / level_host return
LEVEL_CLASSES = 32
LEVEL_DTYPE = np.dtype([("n", "<u8"), ("sumsq", "<u8", (2,)), ("hist", "<u8", (2, LEVEL_CLASSES))])


class Level(C.Structure):
    """gpsbb_level_t: n samples, the sum of x^2 per component, hist[c][k] = components c whose x has bit length k"""
    _fields_ = [("n", C.c_uint64), ("sumsq", C.c_uint64 * 2), ("hist", (C.c_uint64 * LEVEL_CLASSES) * 2)]


assert LEVEL_DTYPE.itemsize == 536 and C.sizeof(Level) == 536


# blind acquisition (include/gpsbb.h gpsbb_device_acquire): the search over PRN, Doppler bin and code delay
ACQ_MAX_BINS, ACQ_PRNS = 64, 32
ACQ_ROW_DTYPE = np.dtype([("peak", "<u8"), ("sum_lo", "<u8"), ("sum_hi", "<u8"), ("lag", "<i4"), ("_pad", "<i4")])


class AcqCfg(C.Structure):
    """gpsbb_acq_cfg_t: prn_mask (bit p-1: PRN p), nbins, step[64] (2^-32 turns per sample), code_step (2^-32 chips per sample),
    ncoh (N), nlags (P), nnc, shift"""
    _fields_ = [("prn_mask", C.c_uint32), ("nbins", C.c_int32), ("step", C.c_int32 * ACQ_MAX_BINS), ("code_step", C.c_uint64),
                ("ncoh", C.c_int32), ("nlags", C.c_int32), ("nnc", C.c_int32), ("shift", C.c_int32)]

    def copy(self, **fields):
        """the same configuration with some fields replaced"""
        c = AcqCfg.from_buffer_copy(self)
        for k, v in fields.items():
            setattr(c, k, v)
        return c


assert ACQ_ROW_DTYPE.itemsize == 32 and C.sizeof(AcqCfg) == 288


# blind tracking (include/gpsbb.h gpsbb_device_track): a carrier and a code loop per channel, epoch by epoch
TRK_LEN, TRK_MAX_CH = 1023 << 32, 32
TRK_STATE_DTYPE = np.dtype([("prn", "<i4"), ("epoch", "<i4"), ("n0", "<i8"), ("carr_phase", "<u4"), ("_pad", "<u4"), ("carr_int", "<i8"),
                            ("carr_step", "<i8"), ("code_phase", "<u8"), ("code_int", "<i8"), ("code_adj", "<i8"), ("prev_i", "<i8"),
                            ("prev_q", "<i8")])
TRK_EPOCH_DTYPE = np.dtype([("n0", "<i8"), ("N", "<i4"), ("q", "<i4"), ("e_i", "<i8"), ("e_q", "<i8"), ("p_i", "<i8"), ("p_q", "<i8"),
                            ("l_i", "<i8"), ("l_q", "<i8"), ("carr_step", "<i8"), ("code_phase", "<u8"), ("carr_phase", "<u4"),
                            ("e_c", "<i4"), ("e_d", "<i4"), ("mode", "<i4")])


class TrkCfg(C.Structure):
    """gpsbb_trk_cfg_t: code_nom (2^-32 chips per sample), aid_div, spacing (2^-32 chips), nfll, kf, kp1, kp2, kd1, kd2, max_epochs"""
    _fields_ = [("code_nom", C.c_uint64), ("aid_div", C.c_int64), ("spacing", C.c_uint32), ("nfll", C.c_int32), ("kf", C.c_int32),
                ("kp1", C.c_int32), ("kp2", C.c_int32), ("kd1", C.c_int32), ("kd2", C.c_int32), ("max_epochs", C.c_int32)]

    def copy(self, **fields):
        """the same configuration with some fields replaced"""
        c = TrkCfg.from_buffer_copy(self)
        for k, v in fields.items():
            setattr(c, k, v)
        return c


assert TRK_STATE_DTYPE.itemsize == 80 and TRK_EPOCH_DTYPE.itemsize == 96 and C.sizeof(TrkCfg) == 48


# the front-end filter (include/gpsbb.h gpsbb_device_fir): a real FIR on I and on Q, one output per `decim` inputs
FIR_MAX_TAPS, FIR_MAX_DECIM, FIR_MAX_SHIFT, FIR_MAX_SUM = 129, 16, 16, 65535
FIR_TILE = 256   # the outputs one of k_fir's workgroups takes (csrc/gpsbb_fir.hip.h; gpsbb_test_fir_tile says the same)


class Fir(C.Structure):
    """gpsbb_fir_t: ntaps, decim, shift, h[0..ntaps-1] with the sum of |h| at most 65535"""
    _fields_ = [("ntaps", C.c_int32), ("decim", C.c_int32), ("shift", C.c_int32), ("_pad", C.c_int32), ("h", C.c_int16 * FIR_MAX_TAPS),
                ("_pad2", C.c_int16)]

    def __init__(self, h=(), decim=1, shift=0):
        super().__init__()
        self.ntaps, self.decim, self.shift = len(h), decim, shift
        for k, v in enumerate(h):
            self.h[k] = v

    def taps(self):
        """h[0..ntaps-1] as int64"""
        return np.array(self.h[:max(int(self.ntaps), 0)], np.int64)


assert C.sizeof(Fir) == 276


# the power spectrum (include/gpsbb.h gpsbb_device_psd): an averaged periodogram of N = 1 << log2n point integer transforms
PSD_MIN_LOG2N, PSD_MAX_LOG2N, PSD_MAX_N, PSD_MAX_HOP, PSD_MAX_SHIFT, PSD_MAX_NSEG = 6, 12, 4096, 1 << 20, 30, 1 << 20
PSD_RECT, PSD_HANN = 0, 1
PSD_MIN_POINTS = 1024    # the points one of k_psd's workgroups holds at least: 1024 / N segments side by side (csrc/gpsbb_psd.hip.h)
PSD_RUN_BATCHES = 2      # a workgroup's run is at least this many loads of its LDS ...
PSD_MAX_WGS = 1024       # ... and longer where the grid would pass this many workgroups


def psd_run(log2n):
    """the segments of a workgroup's least run at N = 1 << log2n (gpsbb_test_psd_run says the same): a call of up to PSD_MAX_WGS
    times as many segments gives every run of that length its own workgroup"""
    return max(1, PSD_MIN_POINTS >> log2n) * PSD_RUN_BATCHES


class Psd(C.Structure):
    """gpsbb_psd_t: log2n, hop, shift, win[0..N-1]"""
    _fields_ = [("log2n", C.c_int32), ("hop", C.c_int32), ("shift", C.c_int32), ("_pad", C.c_int32), ("win", C.c_int16 * PSD_MAX_N)]

    def __init__(self, log2n=PSD_MIN_LOG2N, hop=0, shift=0, win=()):
        super().__init__()
        self.log2n, self.hop, self.shift = log2n, hop, shift
        w = np.ascontiguousarray(win, np.int16)
        C.memmove(self.win, w.ctypes.data, min(w.size, PSD_MAX_N) * 2)

    def window(self):
        """win[0..N-1] as int64"""
        return np.frombuffer(self.win, np.int16, 1 << min(max(int(self.log2n), 0), PSD_MAX_LOG2N)).astype(np.int64)

    def copy(self, **fields):
        c = Psd.from_buffer_copy(self)
        for k, v in fields.items():
            setattr(c, k, v)
        return c


assert C.sizeof(Psd) == 8208


# interference excision (include/gpsbb.h gpsbb_device_excise): half-overlapped segments transformed, bins zeroed, transformed back
EXC_MIN_LOG2N, EXC_MAX_LOG2N, EXC_MAX_N, EXC_WIN_ONE = 6, 12, 4096, 16384
EXC_RUN_BATCHES = 4      # a workgroup's run is at least this many loads of its LDS, less the block it recomputes (csrc/gpsbb_exc.hip.h)


def exc_run(log2n):
    """the blocks (N / 2 samples each) of a workgroup's least run at N = 1 << log2n (gpsbb_test_exc_run says the same)"""
    return max(1, PSD_MIN_POINTS >> log2n) * EXC_RUN_BATCHES - 1


class Exc(C.Structure):
    """gpsbb_exc_t: log2n, thr, win[0..N-1], mask (bit k % 8 of byte k / 8 is bin k)"""
    _fields_ = [("log2n", C.c_int32), ("_pad", C.c_int32), ("thr", C.c_uint64), ("win", C.c_int16 * EXC_MAX_N), ("mask", C.c_uint8 * (EXC_MAX_N // 8))]

    def __init__(self, log2n=EXC_MIN_LOG2N, thr=0, win=(), bins=()):
        super().__init__()
        self.log2n, self.thr = log2n, thr
        w = np.ascontiguousarray(win, np.int16)
        C.memmove(self.win, w.ctypes.data, min(w.size, EXC_MAX_N) * 2)
        self.set_bins(bins)

    def _n(self):
        return 1 << min(max(int(self.log2n), 0), EXC_MAX_LOG2N)

    def window(self):
        """win[0..N-1] as int64"""
        return np.frombuffer(self.win, np.int16, self._n()).astype(np.int64)

    def bins(self):
        """the mask as bool [N], natural bin order"""
        return np.unpackbits(np.frombuffer(self.mask, np.uint8), bitorder="little")[:self._n()].astype(bool)

    def set_bins(self, bins):
        """the mask from bool [N] (or fewer: the rest is cleared)"""
        b = np.zeros(EXC_MAX_N, np.uint8)
        v = np.asarray(bins, bool).ravel()[:EXC_MAX_N]
        b[:v.size] = v
        m = np.packbits(b, bitorder="little")
        C.memmove(self.mask, m.ctypes.data, EXC_MAX_N // 8)

    def copy(self, **fields):
        c = Exc.from_buffer_copy(self)
        for k, v in fields.items():
            if k == "bins":
                c.set_bins(v)
            else:
                setattr(c, k, v)
        return c


assert C.sizeof(Exc) == 8720


# pulse blanking (include/gpsbb.h gpsbb_device_blank): a boxcar power detector in time, the samples around every trigger zeroed
BLANK_MAX_WIN, BLANK_MAX_PRE, BLANK_MAX_HOLD, BLANK_MAX_HIST = 64, 255, 1023, 1341
BLANK_TILE, BLANK_MIN_RUN = 4096, 2   # the outputs of one of k_blank's tiles, the tiles of a workgroup's least run (csrc/gpsbb_blank.h)


class Blank(C.Structure):
    """gpsbb_blank_t: win (L), pre (G), hold, thr"""
    _fields_ = [("win", C.c_int32), ("pre", C.c_int32), ("hold", C.c_int32), ("_pad", C.c_int32), ("thr", C.c_uint64)]

    def __init__(self, win=8, pre=8, hold=8, thr=0):
        super().__init__()
        self.win, self.pre, self.hold, self.thr = win, pre, hold, thr

    def hist(self):
        """K = G + hold + L - 1: the samples of the history"""
        return int(self.pre) + int(self.hold) + int(self.win) - 1

    def copy(self, **fields):
        c = Blank.from_buffer_copy(self)
        for k, v in fields.items():
            setattr(c, k, v)
        return c


assert C.sizeof(Blank) == 24


ERRORS = {0: "GPSBB_OK", -1: "GPSBB_E_BADARG", -2: "GPSBB_E_BADCHAN", -3: "GPSBB_E_HIP", -4: "GPSBB_E_NOMEM",
          -5: "GPSBB_E_INTERNAL", -6: "GPSBB_E_NODEVICE", -7: "GPSBB_E_STATE"}

# every symbol include/gpsbb.h declares
API_SYMBOLS = [
    "gpsbb_create", "gpsbb_destroy", "gpsbb_strerror", "gpsbb_last_hip_error", "gpsbb_version",
    "gpsbb_fill_block", "gpsbb_fill_block_ex", "gpsbb_fill_block_ref", "gpsbb_fill_block_ref_fixed", "gpsbb_batch_create", "gpsbb_batch_destroy",
    "gpsbb_batch_iq_bytes", "gpsbb_batch_run", "gpsbb_sync", "gpsbb_batch_read", "gpsbb_batch_device_iq",
    "gpsbb_get_hazards", "gpsbb_device_read", "gpsbb_device_digest", "gpsbb_slot_digest", "gpsbb_batch_last_timing", "gpsbb_batch_timing_stats", "gpsbb_fill_ceiling", "gpsbb_stream_create",
    "gpsbb_stream_destroy", "gpsbb_stream_push", "gpsbb_stream_pop", "gpsbb_stream_pending", "gpsbb_stream_timing_stats",
    "gpsbb_codegen", "gpsbb_sincos_tables", "gpsbb_chain_carrier_host", "gpsbb_chain_carrier", "gpsbb_set_option",
    "gpsbb_get_info", "gpsbb_stream_reset", "gpsbb_device_affinity", "gpsbb_stream_push_ex", "gpsbb_stream_pop_digest", "gpsbb_host_register", "gpsbb_host_unregister",
    "gpsbb_out_bytes", "gpsbb_device_pack",
    "gpsbb_fill_block_noise", "gpsbb_stream_set_noise", "gpsbb_device_noise", "gpsbb_noise_sigma", "gpsbb_noise_table",
    "gpsbb_despread_segments", "gpsbb_batch_despread", "gpsbb_cn0_estimate",
    "gpsbb_interf_make", "gpsbb_interf_eval", "gpsbb_fill_block_impair", "gpsbb_stream_set_interf", "gpsbb_device_impair",
    "gpsbb_batch_despread_impaired", "gpsbb_batch_despread_lags",
    "gpsbb_device_level", "gpsbb_level_clips", "gpsbb_level_choose", "gpsbb_level_rms", "gpsbb_stream_pop_level",
    "gpsbb_device_acquire", "gpsbb_acq_min_shift", "gpsbb_acq_make", "gpsbb_acq_best",
    "gpsbb_device_track", "gpsbb_trk_make", "gpsbb_trk_seed", "gpsbb_trk_bitsync", "gpsbb_trk_bits",
    "gpsbb_device_fir", "gpsbb_fir_make",
    "gpsbb_device_psd", "gpsbb_psd_make", "gpsbb_psd_min_shift", "gpsbb_psd_twiddles", "gpsbb_psd_scale",
    "gpsbb_device_excise", "gpsbb_exc_make", "gpsbb_exc_from_psd",
    "gpsbb_device_blank", "gpsbb_blank_make", "gpsbb_blank_from_level",
]
# ... and include/gpsbb_node.h
NODE_API_SYMBOLS = ["gpsbb_node_create", "gpsbb_node_run", "gpsbb_node_run_digest", "gpsbb_node_slot_digests", "gpsbb_node_destroy", "gpsbb_node_plan", "gpsbb_node_begin", "gpsbb_node_feed", "gpsbb_node_end",
                    "gpsbb_node_set_noise", "gpsbb_node_set_interf"]


class GpsbbError(RuntimeError):
    def __init__(self, rc, what=""):
        self.rc = rc
        super().__init__("%s failed: %s (%d)" % (what, ERRORS.get(rc, "?"), rc))


def build(force=False):
    """Compile csrc/ for gfx950 with hipcc into libgpsbb.so next to this file (in-tree, so it travels)."""
    if force or not os.path.exists(LIB_PATH) or not os.path.exists(EXP_LIB_PATH) or any(
            os.path.getmtime(os.path.join(HERE, "csrc", f)) > min(os.path.getmtime(LIB_PATH), os.path.getmtime(EXP_LIB_PATH))
            for f in os.listdir(os.path.join(HERE, "csrc"))):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc")])
    return LIB_PATH


_lib = None


def lib():
    """The loaded libgpsbb.so (never a fallback: raises if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libgpsbb.so is not built (run __graft_entry__.build() or make -C %s/csrc)" % HERE)
        L = C.CDLL(LIB_PATH)
        vp, i, d, u = C.c_void_p, C.c_int, C.c_double, C.c_uint
        L.gpsbb_create.argtypes = [C.POINTER(vp), i]
        L.gpsbb_destroy.argtypes = [vp]
        L.gpsbb_destroy.restype = None
        L.gpsbb_strerror.argtypes = [i]
        L.gpsbb_strerror.restype = C.c_char_p
        L.gpsbb_last_hip_error.argtypes = [vp]
        L.gpsbb_set_option.argtypes = [vp, i, C.c_long]
        L.gpsbb_get_info.argtypes = [vp, i, C.POINTER(C.c_uint64)]
        L.gpsbb_fill_block.argtypes = [vp, vp, i, d, i, vp, vp]
        L.gpsbb_fill_block_ex.argtypes = [vp, vp, i, d, i, u, vp, vp]
        L.gpsbb_fill_block_ref.argtypes = [vp, vp, vp, i, vp, d, i, vp]
        L.gpsbb_fill_block_ref_fixed.argtypes = [vp, vp, vp, C.c_size_t, i, vp, d, i, vp]
        L.gpsbb_batch_create.argtypes = [vp, vp, i, i, d, i, u, C.POINTER(vp)]
        L.gpsbb_batch_destroy.argtypes = [vp]
        L.gpsbb_batch_destroy.restype = None
        L.gpsbb_batch_iq_bytes.argtypes = [vp]
        L.gpsbb_batch_iq_bytes.restype = C.c_size_t
        L.gpsbb_batch_run.argtypes = [vp, vp]
        L.gpsbb_sync.argtypes = [vp]
        L.gpsbb_batch_read.argtypes = [vp, vp, vp]
        L.gpsbb_batch_device_iq.argtypes = [vp]
        L.gpsbb_batch_device_iq.restype = vp
        L.gpsbb_get_hazards.argtypes = [vp, vp, i]
        L.gpsbb_device_read.argtypes = [vp, vp, vp, C.c_size_t]
        L.gpsbb_device_digest.argtypes = [vp, vp, C.c_long, C.c_int, vp]
        L.gpsbb_batch_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.gpsbb_batch_timing_stats.argtypes = [vp, C.POINTER(i), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                               C.POINTER(C.c_float), i]
        L.gpsbb_fill_ceiling.argtypes = [vp, vp, C.c_size_t, i, C.POINTER(C.c_float)]
        L.gpsbb_stream_create.argtypes = [vp, i, d, i, i, i, u, C.POINTER(vp)]
        L.gpsbb_stream_destroy.argtypes = [vp]
        L.gpsbb_stream_destroy.restype = None
        L.gpsbb_stream_push.argtypes = [vp, vp]
        L.gpsbb_stream_pop.argtypes = [vp, C.POINTER(vp), vp]
        L.gpsbb_stream_pending.argtypes = [vp]
        L.gpsbb_stream_timing_stats.argtypes = [vp, C.POINTER(i), C.POINTER(C.c_float), C.POINTER(C.c_float), i]
        L.gpsbb_codegen.argtypes = [i, vp]
        L.gpsbb_sincos_tables.argtypes = [vp, vp]
        L.gpsbb_chain_carrier_host.argtypes = [vp, i, i, d, i, vp, i]
        L.gpsbb_chain_carrier.argtypes = [vp, vp, i, i, d, i, vp, vp]
        L.gpsbb_stream_reset.argtypes = [vp]
        L.gpsbb_stream_push_ex.argtypes = [vp, vp, u]
        if hasattr(L, "gpsbb_stream_pop_digest"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_stream_pop_digest.argtypes = [vp, C.POINTER(vp), vp, vp]
        L.gpsbb_device_affinity.argtypes = [i, C.POINTER(i), C.c_char_p, C.c_size_t]
        L.gpsbb_node_create.argtypes = [C.POINTER(vp), vp]
        L.gpsbb_node_destroy.argtypes = [vp]
        L.gpsbb_node_destroy.restype = None
        L.gpsbb_node_run.argtypes = [vp, vp, C.c_long, vp, vp, vp]
        L.gpsbb_node_run_digest.argtypes = [vp, vp, C.c_long, vp, vp]
        L.gpsbb_node_slot_digests.argtypes = [vp, i, vp, i]
        L.gpsbb_slot_digest.argtypes = [vp, vp, C.c_long, C.c_int, vp]
        L.gpsbb_host_register.argtypes = [vp, vp, C.c_size_t]
        L.gpsbb_host_unregister.argtypes = [vp, vp]
        L.gpsbb_node_begin.argtypes = [vp, vp, vp]
        L.gpsbb_node_feed.argtypes = [vp, vp, C.c_long]
        L.gpsbb_node_end.argtypes = [vp, vp]
        L.gpsbb_node_plan.argtypes = [C.c_long, i, i, C.POINTER(C.c_long)]
        L.gpsbb_out_bytes.argtypes = [u, C.c_long]
        L.gpsbb_out_bytes.restype = C.c_long
        L.gpsbb_device_pack.argtypes = [vp, vp, C.c_long, i, u, vp]
        if hasattr(L, "gpsbb_fill_block_noise"):  # the noise calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_fill_block_noise.argtypes = [vp, vp, i, d, i, u, vp, vp, vp]
            L.gpsbb_stream_set_noise.argtypes = [vp, vp]
            L.gpsbb_device_noise.argtypes = [vp, vp, vp, C.c_long, i, vp]
            L.gpsbb_noise_sigma.argtypes = [d, d, d]
            L.gpsbb_noise_sigma.restype = d
            L.gpsbb_noise_table.argtypes = [vp, i]
            L.gpsbb_node_set_noise.argtypes = [vp, vp]
        if hasattr(L, "gpsbb_batch_despread"):  # the despreading calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_despread_segments.argtypes = [C.c_long, i]
            L.gpsbb_despread_segments.restype = C.c_long
            L.gpsbb_batch_despread.argtypes = [vp, vp, u, vp, i, vp]
            L.gpsbb_cn0_estimate.argtypes = [vp, C.c_long, C.c_long, d]
            L.gpsbb_cn0_estimate.restype = d
        if hasattr(L, "gpsbb_interf_eval"):  # the interference calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_interf_make.argtypes = [vp, i, d, d, d, d, d, d, d]
            L.gpsbb_interf_eval.argtypes = [vp, C.c_uint64, C.c_long, vp]
            L.gpsbb_fill_block_impair.argtypes = [vp, vp, i, d, i, u, vp, vp, vp, vp]
            L.gpsbb_stream_set_interf.argtypes = [vp, vp]
            L.gpsbb_device_impair.argtypes = [vp, vp, vp, C.c_long, i, vp, vp]
            L.gpsbb_batch_despread_impaired.argtypes = [vp, vp, u, vp, vp, i, vp]
            L.gpsbb_node_set_interf.argtypes = [vp, vp]
        if hasattr(L, "gpsbb_batch_despread_lags"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_batch_despread_lags.argtypes = [vp, vp, u, vp, vp, i, vp, i, vp]
        if hasattr(L, "gpsbb_device_level"):  # the level calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_device_level.argtypes = [vp, vp, C.c_long, i, vp, vp, vp]
            L.gpsbb_level_clips.argtypes = [vp, C.c_long, i, u, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            L.gpsbb_level_choose.argtypes = [vp, C.c_long, u, d, C.POINTER(i), C.POINTER(i)]
            L.gpsbb_level_rms.argtypes = [vp, C.c_long, i]
            L.gpsbb_level_rms.restype = d
            L.gpsbb_stream_pop_level.argtypes = [vp, C.POINTER(vp), vp, vp]
        if hasattr(L, "gpsbb_device_acquire"):  # the acquisition calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_device_acquire.argtypes = [vp, vp, C.c_long, u, vp, vp, vp, vp, vp]
            L.gpsbb_acq_min_shift.argtypes = [u, i, i]
            L.gpsbb_acq_make.argtypes = [vp, d, d, d, i, d, i, i, u]
            L.gpsbb_acq_best.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_uint64), C.POINTER(d)]
        if hasattr(L, "gpsbb_device_track"):  # the tracking calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_device_track.argtypes = [vp, vp, C.c_long, u, vp, vp, vp, vp, i, vp, vp]
            L.gpsbb_trk_make.argtypes = [vp, d, d, d, d, i, i]
            L.gpsbb_trk_seed.argtypes = [vp, vp, i, i, i]
            L.gpsbb_trk_bitsync.argtypes = [vp, i, i, C.POINTER(i), vp]
            L.gpsbb_trk_bits.argtypes = [vp, i, i, vp, i]
        if hasattr(L, "gpsbb_device_fir"):  # the filter's calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_device_fir.argtypes = [vp, vp, C.c_long, vp, vp, vp, vp, vp, vp, vp]
            L.gpsbb_fir_make.argtypes = [vp, i, i, d, d]
        if hasattr(L, "gpsbb_device_psd"):  # the spectrum's calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_device_psd.argtypes = [vp, vp, C.c_long, u, vp, vp, vp, vp, vp]
            L.gpsbb_psd_make.argtypes = [vp, i, C.c_long, i, C.c_long]
            L.gpsbb_psd_min_shift.argtypes = [C.c_long]
            L.gpsbb_psd_twiddles.argtypes = [vp, vp]
            L.gpsbb_psd_scale.argtypes = [vp, C.c_long, u]
            L.gpsbb_psd_scale.restype = d
        if hasattr(L, "gpsbb_device_excise"):  # the excision's calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_device_excise.argtypes = [vp, vp, C.c_long, vp, vp, vp, vp, vp, vp, vp, vp]
            L.gpsbb_exc_make.argtypes = [vp, i]
            L.gpsbb_exc_from_psd.argtypes = [vp, vp, vp, C.c_long, d, d]
        if hasattr(L, "gpsbb_device_blank"):  # the blanker's calls, as a group (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_device_blank.argtypes = [vp, vp, C.c_long, vp, vp, vp, vp, vp, vp, vp, vp]
            L.gpsbb_blank_make.argtypes = [vp, i, i, i, d, d]
            L.gpsbb_blank_from_level.argtypes = [vp, vp, C.c_long, i, d]
        if hasattr(L, "gpsbb_test_live"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_live.argtypes = [vp]
            L.gpsbb_test_live.restype = None
        _lib = L
    return _lib


_exp_lib = None


def exp_lib():
    """The experiments build (libgpsbb_exp.so) with the gpsbb_test_* hooks of csrc/gpsbb_testhooks.h: the shared NCO code
    (gpsbb_nco.h) compiled for the host, which tests/test_nco_host.py checks against brute-force stepping without a GPU."""
    global _exp_lib
    if _exp_lib is None:
        if not os.path.exists(EXP_LIB_PATH):
            raise RuntimeError("libgpsbb_exp.so is not built (make -C %s/csrc)" % HERE)
        L = C.CDLL(EXP_LIB_PATH)
        i, d, u, vp = C.c_int, C.c_double, C.c_uint, C.c_void_p
        L.gpsbb_test_carr_jump.argtypes = [d, d, C.c_longlong]
        L.gpsbb_test_carr_jump.restype = d
        L.gpsbb_test_code_jump.argtypes = [d, d, C.c_longlong, C.POINTER(C.c_longlong)]
        L.gpsbb_test_code_jump.restype = d
        L.gpsbb_test_build_rows.argtypes = [i, d, d, u, i, vp, i, C.POINTER(d), C.POINTER(u)]
        L.gpsbb_test_row_bound.argtypes = [i, d, i]
        L.gpsbb_test_row_bound.restype = C.c_ulonglong
        L.gpsbb_test_carr_predict.argtypes = [d, d, i]
        L.gpsbb_test_carr_predict.restype = d
        L.gpsbb_test_fixed_tile_index.argtypes = [C.c_uint32, C.c_int32, i]
        L.gpsbb_test_fixed_tile_index.restype = d
        L.gpsbb_test_despread_exact.argtypes = [vp]
        L.gpsbb_test_despread_exact.restype = C.c_ulonglong
        L.gpsbb_test_despread_ms.argtypes = [vp]
        L.gpsbb_test_despread_ms.restype = C.c_float
        if hasattr(L, "gpsbb_test_plan"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_plan.argtypes = [vp, i, i, d, i, u, vp, i, vp, vp, vp, vp, vp]
        if hasattr(L, "gpsbb_test_launch_plan"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_launch_plan.argtypes = [vp, i, i, d, i, u, vp, i, vp, vp, vp, vp, i, i, i, vp]
        if hasattr(L, "gpsbb_test_push_side"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_push_side.argtypes = [vp, i, i, d, i, u, vp, vp]
        if hasattr(L, "gpsbb_test_chain_plan"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_chain_plan.argtypes = [vp, i, i, d, i, i, vp]
        if hasattr(L, "gpsbb_test_fir_ms"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_fir_ms.argtypes = [vp]
            L.gpsbb_test_fir_ms.restype = C.c_float
            L.gpsbb_test_fir_tile.argtypes = []
        if hasattr(L, "gpsbb_test_psd_ms"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_psd_ms.argtypes = [vp]
            L.gpsbb_test_psd_ms.restype = C.c_float
            L.gpsbb_test_psd_run.argtypes = [i]
        if hasattr(L, "gpsbb_test_exc_ms"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_exc_ms.argtypes = [vp]
            L.gpsbb_test_exc_ms.restype = C.c_float
            L.gpsbb_test_exc_run.argtypes = [i]
            L.gpsbb_test_exc_host.argtypes = [vp, vp, C.c_long, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "gpsbb_test_blank_ms"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_blank_ms.argtypes = [vp]
            L.gpsbb_test_blank_ms.restype = C.c_float
            L.gpsbb_test_blank_tile.argtypes = [vp]
            L.gpsbb_test_blank_host.argtypes = [vp, vp, C.c_long, vp, vp, vp, vp, vp]
        if hasattr(L, "gpsbb_test_nav_sign"):  # (an older build loaded for an A/B: tools/ab_lib.sh)
            L.gpsbb_test_nav_sign.argtypes = [C.c_ulonglong, i, i, i, i, vp]
            L.gpsbb_test_nav_sign.restype = None
        _exp_lib = L
    return _exp_lib


def nav_sign(state, minus, g, e=0, used=1):
    """gpsbb_test_nav_sign (csrc/gpsbb_testhooks.h): how a table with a state granule of 2^g tiles keeps a code state (a float64,
    not negative) under a data bit of -1 (minus) or +1, and where a reader finds the bit after a roll-over inside entry e of a row
    of `used` entries.  Returns (stored bit pattern, magnitude's bit pattern, bit, from the end state?, row entry or -1, in the
    sign at all?)."""
    out = np.zeros(6, np.int64)
    exp_lib().gpsbb_test_nav_sign(int(np.float64(state).view(np.uint64)), int(bool(minus)), int(g), int(e), int(used), out.ctypes.data)
    return (int(out[0]) & 0xFFFFFFFFFFFFFFFF, int(out[1]) & 0xFFFFFFFFFFFFFFFF, int(out[2]), bool(out[3]), int(out[4]), bool(out[5]))


PLAN_FIELDS = ("nblocks", "nch", "nsamp", "ntiles", "delt", "flags", "ev", "ev_dense", "ev_all_dense", "laps", "host_seed", "st_log2",
               "nstates", "chain_dev", "chain_starts", "chain_indep", "chain_model", "chain_fix_seq", "nseg", "seg_tiles", "fix_wg",
               "fix_chunks", "nsets", "total_rows", "carr_lanes", "chain_lanes", "cont0_mask", "lap_chunk0", "h_ch", "h_evc", "row_off",
               "h_kph0", "h_kstep", "h_cd", "h_start0", "h_seed_order", "h_chain_order", "carry_phase")


def plan(ch, delt, nsamp, flags=0, seed_where=0, synth_kernel=0, chain_where=0, skip_seed=0, max_sets=6, carry_prn=None,
         carry_phase=None, fixed_prev_prn=None, fixed_prev_phase=None):
    """gpsbb_test_plan (csrc/gpsbb_testhooks.h): what set-up would decide for these descriptors, without a handle or a GPU.  Returns
    (rc, values): values = PLAN_FIELDS -> the BatchPlan scalar, or the 64-bit FNV-1a of the image (0: the plan defines none; `delt`
    is hashed too).  carry_prn / carry_phase (float64, advanced in place): the stream lends its carry; fixed_prev_*: the
    accumulator's chaining state."""
    ch = _as_chan(ch)
    nb, nch = ch.shape
    opt = np.array([seed_where, synth_kernel, skip_seed, chain_where, max_sets], np.int32)
    out = np.zeros(len(PLAN_FIELDS), np.uint64)

    def ptr(a, dtype):
        if a is None:
            return None
        assert a.dtype == dtype and a.flags.c_contiguous and a.size >= nch
        return a.ctypes.data

    rc = exp_lib().gpsbb_test_plan(ch.ctypes.data, nb, nch, delt, nsamp, flags, opt.ctypes.data, int(carry_prn is not None),
                                   ptr(carry_prn, np.int32), ptr(carry_phase, np.float64), ptr(fixed_prev_prn, np.int32),
                                   ptr(fixed_prev_phase, np.uint32), out.ctypes.data)
    return rc, ({f: int(v) for f, v in zip(PLAN_FIELDS, out)} if rc == 0 else None)


LAUNCH_FIELDS = ("prepass", "lap_wide", "lap_merged", "lap_fixed", "chain", "pass_a", "pass_b", "fix_wg", "carr_lanes", "walk_lanes",
                 "chain_order", "seed_ev", "seed_lanes", "ctr_reset", "info_prepass", "variant", "digest_fused", "granule", "ev_chunk",
                 "pd_danger", "helpers", "grid_x", "grid_y", "wg", "lds", "digest_gx", "digest_gy", "last_kernel", "last_chain_dev")
LAUNCH_KERNELS = 16
PREPASS_SKIP, PREPASS_HOST, PREPASS_LAPS, PREPASS_WALKS, PREPASS_SEED = range(5)
# kernel ids of a launch plan: family + 256 * instance (csrc/gpsbb_plan.h: LaunchKernel)
(LK_LAP_PLAN, LK_LAP_PASS1, LK_LAP_SCAN, LK_LAP_PASS2, LK_LAP_REPAIR, LK_LAP_FIXED_TILES, LK_WALK, LK_CHAIN_PREFIX, LK_CHAIN_FIX,
 LK_CHAIN_FIX_PAR, LK_TILES, LK_SEED, LK_BLOCK_DIGEST) = range(1, 14)
LK_SYNTH0 = 100  # + VARIANT_*


def launch_plan(ch, delt, nsamp, flags=0, cus=256, want_digest=0, skip=0, seed_where=0, synth_kernel=0, chain_where=0, skip_seed=0,
                max_sets=6, carry_prn=None, carry_phase=None, fixed_prev_prn=None, fixed_prev_phase=None):
    """gpsbb_test_launch_plan (csrc/gpsbb_testhooks.h): what one run of the batch plan() describes would launch on a device of `cus`
    CUs, without a handle or a GPU.  Returns (rc, values): values = LAUNCH_FIELDS -> the LaunchPlan scalar, and "kernels": the run's
    kernels in order, each [id, grid x, grid y, workgroup, LDS bytes].  The other arguments: as plan()."""
    ch = _as_chan(ch)
    nb, nch = ch.shape
    opt = np.array([seed_where, synth_kernel, skip_seed, chain_where, max_sets], np.int32)
    out = np.zeros(len(LAUNCH_FIELDS) + 1 + 5 * LAUNCH_KERNELS, np.int64)

    def ptr(a, dtype):
        if a is None:
            return None
        assert a.dtype == dtype and a.flags.c_contiguous and a.size >= nch
        return a.ctypes.data

    rc = exp_lib().gpsbb_test_launch_plan(ch.ctypes.data, nb, nch, delt, nsamp, flags, opt.ctypes.data, int(carry_prn is not None),
                                          ptr(carry_prn, np.int32), ptr(carry_phase, np.float64), ptr(fixed_prev_prn, np.int32),
                                          ptr(fixed_prev_phase, np.uint32), cus, int(want_digest), int(skip), out.ctypes.data)
    if rc != 0:
        return rc, None
    nf = len(LAUNCH_FIELDS)
    v = {f: int(x) for f, x in zip(LAUNCH_FIELDS, out)}
    v["kernels"] = [[int(x) for x in out[nf + 1 + 5 * k:nf + 6 + 5 * k]] for k in range(int(out[nf]))]
    return rc, v


PUSH_CHAIN_NONE, PUSH_CHAIN_HOST, PUSH_CHAIN_DEVICE = 0, 1, 2


def push_side(ch, delt, nsamp, flags=0, seed_where=0, synth_kernel=0, chain_where=0, skip_seed=0, max_sets=1):
    """gpsbb_test_push_side (csrc/gpsbb_testhooks.h): on which side a ring with these flags would chain the carrier of this push,
    without a handle or a GPU.  Returns (rc, values): values = {"chain": PUSH_CHAIN_*, "begun": the decision took the plan's first
    step}."""
    ch = _as_chan(ch)
    nb, nch = ch.shape
    opt = np.array([seed_where, synth_kernel, skip_seed, chain_where, max_sets], np.int32)
    out = np.zeros(2, np.int32)
    rc = exp_lib().gpsbb_test_push_side(ch.ctypes.data, nb, nch, delt, nsamp, flags, opt.ctypes.data, out.ctypes.data)
    return rc, ({"chain": int(out[0]), "begun": int(out[1])} if rc == 0 else None)


CHAIN_PLAN_PIECES = 64


def chain_plan(ch, delt, nsamp, seed_where=0, nblocks=None, nch=None):
    """gpsbb_test_chain_plan (csrc/gpsbb_testhooks.h): what gpsbb_chain_carrier would decide for these arguments before its first
    HIP call, without a handle or a GPU.  Returns (rc, values): values = {"laps", "npieces" (the true count), "h_cd", "h_start0"
    (64-bit FNV-1a), "pieces": [[b0, nb, cont0_mask, FNV-1a of chunk0 or 0], ...] (the first CHAIN_PLAN_PIECES)}.  nblocks / nch:
    the counts to pass instead of the array's (the argument checks)."""
    ch = _as_chan(ch)
    nb, nc = ch.shape
    out = np.zeros(4 + 4 * CHAIN_PLAN_PIECES, np.uint64)
    rc = exp_lib().gpsbb_test_chain_plan(ch.ctypes.data, nb if nblocks is None else nblocks, nc if nch is None else nch, delt, nsamp,
                                         seed_where, out.ctypes.data)
    if rc != 0:
        return rc, None
    n = min(int(out[1]), CHAIN_PLAN_PIECES)
    return rc, {"laps": int(out[0]), "npieces": int(out[1]), "h_cd": int(out[2]), "h_start0": int(out[3]),
                "pieces": [[int(v) for v in out[4 + 4 * k:8 + 4 * k]] for k in range(n)]}


def _chk(rc, what):
    if rc != 0:
        raise GpsbbError(rc, what)


def _as_chan(ch):
    ch = np.ascontiguousarray(ch, dtype=CHAN_DTYPE)
    if ch.ndim == 1:
        ch = ch[None, :]
    if ch.ndim != 2:
        raise ValueError("descriptors must be [nblocks, nch]")
    return ch


# ---- host helpers ------------------------------------------------------------------------------------

def codegen(prn):
    ca = np.zeros(1023, np.uint8)
    _chk(lib().gpsbb_codegen(prn, ca.ctypes.data), "gpsbb_codegen")
    return ca


def sincos_tables():
    s = np.zeros(512, np.int32)
    c = np.zeros(512, np.int32)
    _chk(lib().gpsbb_sincos_tables(s.ctypes.data, c.ctypes.data), "gpsbb_sincos_tables")
    return s, c


def chain_carrier_host(ch, delt, nsamp, nthreads=0):
    ch = _as_chan(ch)
    nb, nch = ch.shape
    seed = np.zeros((nb, nch), np.float64)
    _chk(lib().gpsbb_chain_carrier_host(ch.ctypes.data, nb, nch, delt, nsamp, seed.ctypes.data, nthreads),
         "gpsbb_chain_carrier_host")
    return seed


# ---- device objects ----------------------------------------------------------------------------------

class Synth:
    """One libgpsbb handle: one GPU, one producer thread (gpsbb_create / gpsbb_destroy)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _chk(lib().gpsbb_create(C.byref(self._h), device), "gpsbb_create")

    def close(self):
        if self._h:
            lib().gpsbb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def fill_block(self, ch, delt, nsamp, flags=0, out=None, fmt=OUT_SC16, noise=None, interf=None):
        """gpsbb_fill_block(_ex): ch = CHAN_DTYPE[nch] -> (int16 [nsamp,2], STATE_DTYPE[nch]); out: the caller's iq_buff.
        fmt (OUT_SC8(shift) / OUT_SC1): the block comes back packed — int8 [nsamp, 2] / uint8 [nsamp // 4] — and `out`, if given,
        is any C-contiguous array of at least out_bytes(fmt, nsamp) bytes (a registered iq_buff: written straight into).
        noise (a Noise or a dict: seed, sigma, sample0, shift): gpsbb_fill_block_noise.
        interf (an InterfSet or a dict: emitters, shift, sample0): gpsbb_fill_block_impair, with or without noise."""
        ch = np.ascontiguousarray(ch, dtype=CHAN_DTYPE)
        if fmt & (OUT_FORMAT_MASK | OUT_SHIFT_MASK):
            nbytes = out_bytes(fmt, nsamp)
            buf = np.empty(nbytes, np.uint8) if out is None else out
            assert buf.flags.c_contiguous and buf.nbytes >= nbytes
        else:
            buf = np.empty((nsamp, 2), np.int16) if out is None else out
            assert buf.dtype == np.int16 and buf.flags.c_contiguous and buf.size >= 2 * nsamp
        st = np.zeros(ch.shape[0], STATE_DTYPE)
        nz = _as_noise(noise)
        js = _as_interf(interf)
        if js is not None:
            _chk(lib().gpsbb_fill_block_impair(self._h, ch.ctypes.data, ch.shape[0], delt, nsamp, flags | fmt, _ref(nz), C.byref(js),
                                               buf.ctypes.data, st.ctypes.data), "gpsbb_fill_block_impair")
        elif nz is not None:
            _chk(lib().gpsbb_fill_block_noise(self._h, ch.ctypes.data, ch.shape[0], delt, nsamp, flags | fmt, C.byref(nz),
                                              buf.ctypes.data, st.ctypes.data), "gpsbb_fill_block_noise")
        else:
            _chk(lib().gpsbb_fill_block_ex(self._h, ch.ctypes.data, ch.shape[0], delt, nsamp, flags | fmt, buf.ctypes.data,
                                           st.ctypes.data), "gpsbb_fill_block_ex")
        if fmt & (OUT_FORMAT_MASK | OUT_SHIFT_MASK):
            return _as_out(buf, 1, nsamp, fmt)[0], st
        return buf, st

    def fill_block_ref(self, chan, gain, delt, nsamp, iq, layout=None):
        """gpsbb_fill_block_ref: the reference's own channel_t[] (REF_CHANNEL_DTYPE, updated in place like the loop does,
        c:2709-2746) and gain[]; iq: int16 [nsamp, 2], the caller's iq_buff (c:84)"""
        layout = layout or ref_layout(chan.dtype)
        _chk(lib().gpsbb_fill_block_ref(self._h, chan.ctypes.data, C.byref(layout), chan.shape[0], gain.ctypes.data, delt, nsamp,
                                        iq.ctypes.data), "gpsbb_fill_block_ref")

    def host_register(self, arr):
        """gpsbb_host_register: fills into `arr` (the caller's iq_buff, kept alive by the caller) are rendered straight into it"""
        _chk(lib().gpsbb_host_register(self._h, arr.ctypes.data, arr.nbytes), "gpsbb_host_register")

    def host_unregister(self, arr):
        _chk(lib().gpsbb_host_unregister(self._h, arr.ctypes.data), "gpsbb_host_unregister")

    def batch(self, ch, delt, nsamp, flags=0):
        return Batch(self, ch, delt, nsamp, flags)

    def stream(self, nch, delt, nsamp, blocks_per_slot, depth=3, flags=0, fmt=OUT_SC16, noise=None, interf=None):
        return Stream(self, nch, delt, nsamp, blocks_per_slot, depth, flags, fmt, noise, interf)

    def device_impair(self, d_src, nblocks, nsamp, noise, interf, d_dst=None):
        """gpsbb_device_impair: as device_noise, with the set's interference added; noise may be None"""
        nz, js = _as_noise(noise), _as_interf(interf)
        dst = d_src if d_dst is None else d_dst
        _chk(lib().gpsbb_device_impair(self._h, C.c_void_p(int(d_src)), C.c_void_p(int(dst)), nblocks, nsamp, _ref(nz), _ref(js)),
             "gpsbb_device_impair")

    def device_level(self, d_ptr, nblocks, nsamp, noise=None, interf=None):
        """gpsbb_device_level: the level of x = v + N + J before the shift, of nblocks blocks of int16 IQ in device memory ->
        LEVEL_DTYPE [nblocks] (level_host is the same in numpy); noise and interf may each be None"""
        nz, js = _as_noise(noise), _as_interf(interf)
        out = np.zeros(nblocks, LEVEL_DTYPE)
        _chk(lib().gpsbb_device_level(self._h, C.c_void_p(int(d_ptr)), nblocks, nsamp, _ref(nz), _ref(js), out.ctypes.data),
             "gpsbb_device_level")
        return out

    def device_acquire(self, d_ptr, nsamp, cfg, view=OUT_SC16, noise=None, interf=None, want_grid=False):
        """gpsbb_device_acquire: the search of nsamp int16 I/Q pairs in device memory -> rows ACQ_ROW_DTYPE [32, nbins], or
        (rows, grid uint64 [32, nbins, nlags]) with want_grid (acquire_host is the same in numpy)"""
        nz, js = _as_noise(noise), _as_interf(interf)
        rows = np.zeros((ACQ_PRNS, max(int(cfg.nbins), 0)), ACQ_ROW_DTYPE)
        grid = np.zeros((ACQ_PRNS, max(int(cfg.nbins), 0), max(int(cfg.nlags), 0)), np.uint64) if want_grid else None
        _chk(lib().gpsbb_device_acquire(self._h, C.c_void_p(int(d_ptr)), int(nsamp), view, _ref(nz), _ref(js), C.byref(cfg),
                                        rows.ctypes.data, None if grid is None else grid.ctypes.data), "gpsbb_device_acquire")
        return (rows, grid) if want_grid else rows

    def device_track(self, d_ptr, nsamp, cfg, states, view=OUT_SC16, noise=None, interf=None):
        """gpsbb_device_track: the channels of `states` (TRK_STATE_DTYPE [nch], left as they are) followed through nsamp int16 I/Q
        pairs in device memory -> (the states after, TRK_STATE_DTYPE [nch]; per channel its records, a list of TRK_EPOCH_DTYPE
        arrays).  track_host is the same in numpy"""
        nz, js = _as_noise(noise), _as_interf(interf)
        st = np.array(states, TRK_STATE_DTYPE).reshape(-1)
        nch = st.size
        # (no more records than epochs can fit the buffer: every epoch after a channel's first has more than LEN / cs - 1 samples.
        # The call lays the records out as [nch][max_epochs], so it is handed the smaller number: the same records)
        cs_max = int(cfg.code_nom) + int(cfg.code_nom) // 8
        fit = 2 + max(int(nsamp), 0) // max(1, TRK_LEN // max(cs_max, 1) - 1)
        if 1 <= int(cfg.max_epochs) and fit < int(cfg.max_epochs):
            cfg = cfg.copy(max_epochs=fit)
        room = np.zeros((nch, max(int(cfg.max_epochs), 1)), TRK_EPOCH_DTYPE)
        counts = np.zeros(max(nch, 1), np.int32)
        _chk(lib().gpsbb_device_track(self._h, C.c_void_p(int(d_ptr)), int(nsamp), view, _ref(nz), _ref(js), C.byref(cfg), st.ctypes.data, nch,
                                      room.ctypes.data, counts.ctypes.data), "gpsbb_device_track")
        return st, [room[c, :int(counts[c])].copy() for c in range(nch)]

    def device_fir(self, d_ptr, nsamp, fir, d_out, hist=None, noise=None, interf=None):
        """gpsbb_device_fir: nsamp int16 I/Q pairs in device memory at d_ptr, filtered and decimated into nsamp / fir.decim pairs at
        d_out -> (the history to hand to the next call, int16 [ntaps - 1, 2]; the components the clamp changed).  hist: the
        history a call before returned, or None (zeros).  fir_host over view_host's output is the same in numpy"""
        nz, js = _as_noise(noise), _as_interf(interf)
        nh = max(int(fir.ntaps) - 1, 0)
        hin = None if hist is None else np.ascontiguousarray(hist, np.int16).reshape(nh, 2)
        hout = np.zeros((nh, 2), np.int16)
        clipped = C.c_uint64(0)
        _chk(lib().gpsbb_device_fir(self._h, C.c_void_p(int(d_ptr)), int(nsamp), _ref(nz), _ref(js), C.byref(fir),
                                    None if hin is None else hin.ctypes.data, hout.ctypes.data, C.c_void_p(int(d_out)), C.byref(clipped)),
             "gpsbb_device_fir")
        return hout, int(clipped.value)

    def device_psd(self, d_ptr, nsamp, psd, view=OUT_SC16, noise=None, interf=None):
        """gpsbb_device_psd: the power spectrum of the view `view` of nsamp int16 I/Q pairs in device memory at d_ptr under the plan
        psd (a Psd) -> (uint64 [N] in natural bin order, the segments).  psd_host over view_host's output is the same in numpy"""
        nz, js = _as_noise(noise), _as_interf(interf)
        out = np.zeros(1 << min(max(int(psd.log2n), 0), PSD_MAX_LOG2N), np.uint64)
        nseg = C.c_long(0)
        _chk(lib().gpsbb_device_psd(self._h, C.c_void_p(int(d_ptr)), int(nsamp), view, _ref(nz), _ref(js), C.byref(psd), out.ctypes.data,
                                    C.byref(nseg)), "gpsbb_device_psd")
        return out, int(nseg.value)

    def device_excise(self, d_ptr, nsamp, exc, d_out, hist=None, noise=None, interf=None):
        """gpsbb_device_excise: nsamp int16 I/Q pairs in device memory at d_ptr, the bins the plan exc (an Exc) names taken out,
        into nsamp pairs at d_out, delayed by N / 2 -> (the history to hand to the next call, int16 [N, 2]; the components the
        clamp changed; the (segment, bin) pairs zeroed).  hist: the history a call before returned, or None (zeros).  excise_host
        over view_host's output is the same in numpy"""
        nz, js = _as_noise(noise), _as_interf(interf)
        N = 1 << min(max(int(exc.log2n), 0), EXC_MAX_LOG2N)
        hin = None if hist is None else np.ascontiguousarray(hist, np.int16).reshape(N, 2)
        hout = np.zeros((N, 2), np.int16)
        clipped, excised = C.c_uint64(0), C.c_uint64(0)
        _chk(lib().gpsbb_device_excise(self._h, C.c_void_p(int(d_ptr)), int(nsamp), _ref(nz), _ref(js), C.byref(exc),
                                       None if hin is None else hin.ctypes.data, hout.ctypes.data, C.c_void_p(int(d_out)), C.byref(clipped),
                                       C.byref(excised)), "gpsbb_device_excise")
        return hout, int(clipped.value), int(excised.value)

    def device_blank(self, d_ptr, nsamp, blank, d_out, hist=None, noise=None, interf=None):
        """gpsbb_device_blank: nsamp int16 I/Q pairs in device memory at d_ptr, the samples around every trigger of the plan blank
        (a Blank) zeroed, into nsamp pairs at d_out, delayed by blank.pre -> (the history to hand to the next call, int16 [K, 2];
        the outputs zeroed; the triggers).  hist: the history a call before returned, or None (zeros).  blank_host over view_host's
        output is the same in numpy"""
        nz, js = _as_noise(noise), _as_interf(interf)
        K = min(max(blank.hist(), 0), BLANK_MAX_HIST)
        hin = None if hist is None else np.ascontiguousarray(hist, np.int16).reshape(K, 2)
        hout = np.zeros((K, 2), np.int16)
        blanked, triggers = C.c_uint64(0), C.c_uint64(0)
        _chk(lib().gpsbb_device_blank(self._h, C.c_void_p(int(d_ptr)), int(nsamp), _ref(nz), _ref(js), C.byref(blank),
                                      None if hin is None or K == 0 else hin.ctypes.data, hout.ctypes.data if K else None, C.c_void_p(int(d_out)),
                                      C.byref(blanked), C.byref(triggers)), "gpsbb_device_blank")
        return hout, int(blanked.value), int(triggers.value)

    def device_noise(self, d_src, nblocks, nsamp, noise, d_dst=None):
        """gpsbb_device_noise: nblocks blocks of int16 IQ in device memory at d_src, with noise, into d_dst (default: in place)"""
        nz = _as_noise(noise)
        dst = d_src if d_dst is None else d_dst
        _chk(lib().gpsbb_device_noise(self._h, C.c_void_p(int(d_src)), C.c_void_p(int(dst)), nblocks, nsamp,
                                      None if nz is None else C.byref(nz)), "gpsbb_device_noise")

    def device_pack(self, d_ptr, nblocks, nsamp, fmt, out=None):
        """gpsbb_device_pack: nblocks blocks of int16 IQ in device memory, packed into host memory in format fmt -> the array of
        iq_view's shape; out: a C-contiguous host array (pageable or pinned) of at least nblocks * out_bytes(fmt, nsamp) bytes"""
        nbytes = nblocks * out_bytes(fmt, nsamp)
        buf = np.empty(nbytes, np.uint8) if out is None else out
        assert buf.flags.c_contiguous and buf.nbytes >= nbytes
        _chk(lib().gpsbb_device_pack(self._h, C.c_void_p(int(d_ptr)), nblocks, nsamp, fmt, buf.ctypes.data), "gpsbb_device_pack")
        return _as_out(buf, nblocks, nsamp, fmt)

    def sync(self):
        _chk(lib().gpsbb_sync(self._h), "gpsbb_sync")

    def device_read(self, d_ptr, shape, dtype=np.int16):
        """gpsbb_device_read: a numpy array filled from device memory the library handed out"""
        out = np.empty(shape, dtype)
        _chk(lib().gpsbb_device_read(self._h, out.ctypes.data, d_ptr, out.nbytes), "gpsbb_device_read")
        return out

    def slot_digest(self, d_ptr, nblocks, nsamp):
        """gpsbb_slot_digest: digests of a slot known to be complete (what pop returned), without draining the handle"""
        out = np.zeros(nblocks, np.uint64)
        _chk(lib().gpsbb_slot_digest(self._h, C.c_void_p(int(d_ptr)), nblocks, nsamp, out.ctypes.data), "gpsbb_slot_digest")
        return out

    def device_digest(self, d_ptr, nblocks, nsamp):
        """gpsbb_device_digest: one uint64 per block of IQ in device memory (see block_digest_host)"""
        out = np.empty(nblocks, np.uint64)
        for k0 in range(0, nblocks, 65535):
            n = min(65535, nblocks - k0)
            _chk(lib().gpsbb_device_digest(self._h, d_ptr + k0 * nsamp * 4, n, nsamp, out[k0:].ctypes.data), "gpsbb_device_digest")
        return out

    def hazards(self, reset=False):
        v = np.zeros(2, np.uint64)
        _chk(lib().gpsbb_get_hazards(self._h, v.ctypes.data, int(reset)), "gpsbb_get_hazards")
        return {"itable_512": int(v[0]), "dwrd_oob": int(v[1])}

    def set_option(self, option, value):
        """gpsbb_set_option: OPT_SEED_WHERE / OPT_SYNTH_KERNEL / OPT_SKIP_SEED (per handle)"""
        _chk(lib().gpsbb_set_option(self._h, option, value), "gpsbb_set_option")

    def info(self, what):
        """gpsbb_get_info: INFO_LAST_KERNEL / INFO_EXACT_RUNS"""
        v = C.c_uint64()
        _chk(lib().gpsbb_get_info(self._h, what, C.byref(v)), "gpsbb_get_info")
        return int(v.value)

    def chain_carrier(self, ch, delt, nsamp, want_seeds=True):
        """gpsbb_chain_carrier: the exact carrier chain on the device, nothing rendered -> (start phase of every block
        [nblocks, nch] or None, phase after the last block [nch])"""
        ch = _as_chan(ch)
        nb, nch = ch.shape
        seed = np.zeros((nb, nch), np.float64) if want_seeds else None
        end = np.zeros(nch, np.float64)
        _chk(lib().gpsbb_chain_carrier(self._h, ch.ctypes.data, nb, nch, delt, nsamp,
                                       seed.ctypes.data if want_seeds else None, end.ctypes.data), "gpsbb_chain_carrier")
        return seed, end

    def shard_seed(self, ch, b0, delt, nsamp):
        """The exact carr_phase block b0 of the stream `ch` starts from (per channel): the end of the device-side chain
        over the blocks before it for a channel that keeps its prn, the descriptor's own phase otherwise."""
        ch = _as_chan(ch)
        if b0 == 0:
            return ch["carr_phase"][0].copy()
        _, end = self.chain_carrier(ch[:b0], delt, nsamp, want_seeds=False)
        cont = (ch["prn"][b0] > 0) & (ch["prn"][b0] == ch["prn"][b0 - 1])
        return np.where(cont, end, ch["carr_phase"][b0])

    def fill_ceiling(self, d_ptr, nbytes, iters=10):
        ms = C.c_float()
        _chk(lib().gpsbb_fill_ceiling(self._h, d_ptr, nbytes, iters, C.byref(ms)), "gpsbb_fill_ceiling")
        return ms.value


class Batch:
    """Block descriptors resident in HBM (gpsbb_batch_*)."""

    def __init__(self, synth, ch, delt, nsamp, flags=0):
        ch = _as_chan(ch)
        self.synth = synth
        self.nblocks, self.nch = ch.shape
        self.nsamp = nsamp
        self._b = C.c_void_p()
        _chk(lib().gpsbb_batch_create(synth._h, ch.ctypes.data, self.nblocks, self.nch, delt, nsamp, flags,
                                      C.byref(self._b)), "gpsbb_batch_create")

    def close(self):
        if self._b:
            lib().gpsbb_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def iq_bytes(self):
        return lib().gpsbb_batch_iq_bytes(self._b)

    def run(self, d_iq=None):
        """Enqueue seeding pre-pass + synthesis; d_iq = device pointer (int) or None for the internal buffer."""
        _chk(lib().gpsbb_batch_run(self._b, d_iq), "gpsbb_batch_run")

    def read(self, want_iq=True):
        iq = np.empty((self.nblocks, self.nsamp, 2), np.int16) if want_iq else None
        st = np.zeros((self.nblocks, self.nch), STATE_DTYPE)
        _chk(lib().gpsbb_batch_read(self._b, iq.ctypes.data if want_iq else None, st.ctypes.data),
             "gpsbb_batch_read")
        return iq, st

    def timing(self):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        _chk(lib().gpsbb_batch_last_timing(self._b, C.byref(a), C.byref(b), C.byref(c)), "gpsbb_batch_last_timing")
        return {"ms_seed": a.value, "ms_synth": b.value, "ms_total": c.value}

    def timing_stats(self, reset=True):
        n, a, b, c = C.c_int(), C.c_float(), C.c_float(), C.c_float()
        _chk(lib().gpsbb_batch_timing_stats(self._b, C.byref(n), C.byref(a), C.byref(b), C.byref(c), int(reset)),
             "gpsbb_batch_timing_stats")
        return {"runs": n.value, "ms_seed_sum": a.value, "ms_synth_sum": b.value, "ms_total_sum": c.value}

    def device_iq(self):
        return lib().gpsbb_batch_device_iq(self._b)

    def level(self, noise=None, interf=None, d_iq=None):
        """gpsbb_device_level of the batch's blocks: on device_iq() (the last run's internal buffer) unless d_iq is given"""
        p = self.device_iq() if d_iq is None else d_iq
        if not p:
            raise GpsbbError(-7, "Batch.level (no internal buffer: run() first, or pass d_iq)")
        return self.synth.device_level(p, self.nblocks, self.nsamp, noise, interf)

    def despread(self, view=OUT_SC16, noise=None, seg_tiles=1, d_iq=None, interf=None):
        """gpsbb_batch_despread: the prompt sums of every channel of the last run against its own replica, in the receiver's
        view `view` (OUT_SC16 / OUT_SC8(shift) / OUT_SC1) of the rendered IQ, with `noise` (a Noise or a dict) applied first;
        d_iq: a device pointer (int) to the blocks, None: the last run's internal buffer -> int64 [nblocks, nch, nseg, 2] (P.i, P.q)"""
        nseg = despread_segments(self.nsamp, seg_tiles)
        out = np.zeros((self.nblocks, self.nch, nseg, 2), np.int64)
        nz = _as_noise(noise)
        js = _as_interf(interf)
        if js is not None:  # gpsbb_batch_despread_impaired: the set's J added in the view
            _chk(lib().gpsbb_batch_despread_impaired(self._b, None if d_iq is None else C.c_void_p(int(d_iq)), view, _ref(nz),
                                                     C.byref(js), seg_tiles, out.ctypes.data), "gpsbb_batch_despread_impaired")
            return out
        _chk(lib().gpsbb_batch_despread(self._b, None if d_iq is None else C.c_void_p(int(d_iq)), view,
                                        None if nz is None else C.byref(nz), seg_tiles, out.ctypes.data), "gpsbb_batch_despread")
        return out

    def despread_lags(self, lags, seg_tiles=1, view=OUT_SC16, noise=None, interf=None, d_iq=None):
        """gpsbb_batch_despread_lags: despread's sums with the view taken `lags[l]` samples later than the replica (within
        the block: zero outside it) -> int64 [nblocks, nch, nseg, nlags, 2]; the column of a lag 0 is despread's result"""
        lg = np.ascontiguousarray(lags, np.int32).reshape(-1)
        nseg = despread_segments(self.nsamp, seg_tiles)
        out = np.zeros((self.nblocks, self.nch, nseg, lg.size, 2), np.int64)
        nz = _as_noise(noise)
        js = _as_interf(interf)
        _chk(lib().gpsbb_batch_despread_lags(self._b, None if d_iq is None else C.c_void_p(int(d_iq)), view, _ref(nz), _ref(js),
                                             seg_tiles, lg.ctypes.data, lg.size, out.ctypes.data), "gpsbb_batch_despread_lags")
        return out


class Stream:
    """Time-sharded streaming with pinned host gather (gpsbb_stream_*)."""

    def __init__(self, synth, nch, delt, nsamp, blocks_per_slot, depth=3, flags=0, fmt=OUT_SC16, noise=None, interf=None):
        self.synth = synth
        self.nch, self.nsamp, self.bps = nch, nsamp, blocks_per_slot
        self.device_only = bool(flags & STREAM_DEVICE_ONLY)
        self.fmt = fmt  # OUT_SC8(shift) / OUT_SC1: pop() hands out the slot's packed bytes (iq_view's shape)
        self._s = C.c_void_p()
        _chk(lib().gpsbb_stream_create(synth._h, nch, delt, nsamp, blocks_per_slot, depth, flags | fmt,
                                       C.byref(self._s)), "gpsbb_stream_create")
        if noise is not None:
            self.set_noise(noise)
        if interf is not None:
            self.set_interf(interf)

    def set_interf(self, interf):
        """gpsbb_stream_set_interf: interference on the host gather from the next push on (that push at the set's sample0);
        None: off"""
        _chk(lib().gpsbb_stream_set_interf(self._s, _ref(_as_interf(interf))), "gpsbb_stream_set_interf")

    def set_noise(self, noise):
        """gpsbb_stream_set_noise: noise on the host gather from the next push on (that push at noise's sample0); None: off"""
        nz = _as_noise(noise)
        _chk(lib().gpsbb_stream_set_noise(self._s, None if nz is None else C.byref(nz)), "gpsbb_stream_set_noise")

    def close(self):
        if self._s:
            lib().gpsbb_stream_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, ch, new_chain=False, digest=False, level=False):
        """gpsbb_stream_push(_ex); digest: GPSBB_PUSH_DIGEST — the push is rendered with its blocks' digests (pop_digest);
        level: GPSBB_PUSH_LEVEL — the push's slot is measured with the stream's noise and set (pop_level)"""
        ch = _as_chan(ch)
        if ch.shape != (self.bps, self.nch):
            raise ValueError("push expects [blocks_per_slot, nch] descriptors")
        flags = (PUSH_NEW_CHAIN if new_chain else 0) | (PUSH_DIGEST if digest else 0) | (PUSH_LEVEL if level else 0)
        if flags:
            _chk(lib().gpsbb_stream_push_ex(self._s, ch.ctypes.data, flags), "gpsbb_stream_push_ex")
        else:
            _chk(lib().gpsbb_stream_push(self._s, ch.ctypes.data), "gpsbb_stream_push")

    def pop_digest(self, copy=True):
        """gpsbb_stream_pop_digest: pop() plus the popped push's block digests (uint64 [blocks_per_slot])"""
        p = C.c_void_p()
        st = np.zeros((self.bps, self.nch), STATE_DTYPE)
        dig = np.zeros(self.bps, np.uint64)
        _chk(lib().gpsbb_stream_pop_digest(self._s, C.byref(p), st.ctypes.data, dig.ctypes.data), "gpsbb_stream_pop_digest")
        if self.device_only:
            return p.value, st, dig
        view = iq_view(p.value, self.bps, self.nsamp, self.fmt)
        return (view.copy() if copy else view), st, dig

    def pop_level(self, copy=True):
        """gpsbb_stream_pop_level: pop() plus the popped push's levels (LEVEL_DTYPE [blocks_per_slot])"""
        p = C.c_void_p()
        st = np.zeros((self.bps, self.nch), STATE_DTYPE)
        lv = np.zeros(self.bps, LEVEL_DTYPE)
        _chk(lib().gpsbb_stream_pop_level(self._s, C.byref(p), st.ctypes.data, lv.ctypes.data), "gpsbb_stream_pop_level")
        view = iq_view(p.value, self.bps, self.nsamp, self.fmt)
        return (view.copy() if copy else view), st, lv

    def pop(self, copy=True):
        """(IQ [blocks_per_slot, nsamp, 2] int16 in the slot's pinned host buffer, end states); a stream created with
        STREAM_DEVICE_ONLY returns the slot's device pointer (an int) instead of the array."""
        p = C.c_void_p()
        st = np.zeros((self.bps, self.nch), STATE_DTYPE)
        _chk(lib().gpsbb_stream_pop(self._s, C.byref(p), st.ctypes.data), "gpsbb_stream_pop")
        if self.device_only:
            return p.value, st
        view = iq_view(p.value, self.bps, self.nsamp, self.fmt)
        return (view.copy() if copy else view), st

    @property
    def pending(self):
        return lib().gpsbb_stream_pending(self._s)

    def reset(self):
        """gpsbb_stream_reset: a new stream on the same ring (every slot popped); the next push is block 0 again"""
        _chk(lib().gpsbb_stream_reset(self._s), "gpsbb_stream_reset")

    def timing_stats(self, reset=True):
        n, a, b = C.c_int(), C.c_float(), C.c_float()
        _chk(lib().gpsbb_stream_timing_stats(self._s, C.byref(n), C.byref(a), C.byref(b), int(reset)),
             "gpsbb_stream_timing_stats")
        return {"runs": n.value, "ms_seed_sum": a.value, "ms_synth_sum": b.value}


# ---- synthetic descriptors (BASELINE / SURVEY section 8d, workload M2) -------------------------------

# ---- include/gpsbb_node.h: one process, N handles, one sink ------------------------------------------

class _NodeConfig(C.Structure):
    _fields_ = [("nshards", C.c_int), ("devices", C.POINTER(C.c_int)), ("nch", C.c_int), ("delt", C.c_double), ("nsamp", C.c_int),
                ("blocks_per_slot", C.c_int), ("depth", C.c_int), ("flags", C.c_uint)]


class _NodeShardStats(C.Structure):
    _fields_ = [("first_block", C.c_long), ("nblocks", C.c_long), ("device", C.c_int), ("numa_node", C.c_int), ("cpus_bound", C.c_int),
                ("seed_seconds", C.c_double), ("busy_seconds", C.c_double), ("wait_seconds", C.c_double)]


class _NodeStats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("blocks", C.c_long), ("nshards", C.c_int), ("shard", _NodeShardStats * NODE_MAX_SHARDS)]


NODE_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int)


def node_plan(nblocks, nshards, blocks_per_slot):
    first = (C.c_long * (nshards + 1))()
    _chk(lib().gpsbb_node_plan(nblocks, nshards, blocks_per_slot, first), "gpsbb_node_plan")
    return list(first)


def device_affinity(device):
    """gpsbb_device_affinity -> (numa node, "cpu list")"""
    node = C.c_int(-1)
    buf = C.create_string_buffer(512)
    _chk(lib().gpsbb_device_affinity(device, C.byref(node), buf, 512), "gpsbb_device_affinity")
    return node.value, buf.value.decode()


class Node:
    """gpsbb_node_*: nshards producer threads (one handle + one ring each, bound next to their GPU), one sink."""

    def __init__(self, nshards, nch, delt, nsamp, blocks_per_slot, depth=3, flags=0, devices=None, fmt=OUT_SC16, noise=None,
                 interf=None):
        self.nshards, self.nch, self.nsamp = nshards, nch, nsamp
        self.fmt = fmt  # OUT_SC8(shift) / OUT_SC1: the sink's iq points at packed bytes (iq_view(iq, nblocks, nsamp, fmt))
        dev = (C.c_int * nshards)(*(devices if devices is not None else range(nshards)))
        cfg = _NodeConfig(nshards, dev, nch, delt, nsamp, blocks_per_slot, depth, flags | fmt)
        self._n = C.c_void_p()
        _chk(lib().gpsbb_node_create(C.byref(self._n), C.byref(cfg)), "gpsbb_node_create")
        if noise is not None:
            self.set_noise(noise)
        if interf is not None:
            self.set_interf(interf)

    def set_interf(self, interf):
        """gpsbb_node_set_interf: block b of every later run at stream position the set's sample0 + b * nsamp; None: off"""
        _chk(lib().gpsbb_node_set_interf(self._n, _ref(_as_interf(interf))), "gpsbb_node_set_interf")

    def set_noise(self, noise):
        """gpsbb_node_set_noise: block b of every later run at stream position noise's sample0 + b * nsamp; None: off"""
        nz = _as_noise(noise)
        _chk(lib().gpsbb_node_set_noise(self._n, None if nz is None else C.byref(nz)), "gpsbb_node_set_noise")

    def close(self):
        if self._n:
            lib().gpsbb_node_destroy(self._n)
            self._n = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, ch, sink, expect_stop=False):
        """sink(iq_ptr, first_block, nblocks, shard) -> int (< 0 stops); returns the run's statistics as a dict.
        sink may also be a C function pointer (int) for a sink that lives in native code."""
        ch = _as_chan(ch)
        if ch.ndim != 2 or ch.shape[1] != self.nch:
            raise ValueError("descriptors of shape (nblocks, %d) wanted, got %r" % (self.nch, ch.shape))  # (C would read out of bounds)
        raised = []
        if callable(sink):
            def guarded(user, iq, first, nb, shard):
                # an exception must not vanish inside ctypes (which would turn it into "return 0": the run goes on as if the
                # sink were fine): it stops the run and comes back out of Node.run
                try:
                    return int(sink(iq, first, nb, shard) or 0)
                except BaseException as e:  # noqa: BLE001
                    raised.append(e)
                    return -1
            cb = NODE_SINK(guarded)
            fn = C.cast(cb, C.c_void_p)
        else:
            cb, fn = None, C.c_void_p(sink)
        st = _NodeStats()
        rc = lib().gpsbb_node_run(self._n, ch.ctypes.data, ch.shape[0], fn, None, C.byref(st))
        del cb
        if raised:
            raise raised[0]
        if rc != 0 and not (expect_stop and rc == -7):
            raise GpsbbError(rc, "gpsbb_node_run")
        return {"rc": rc, "seconds": st.seconds, "blocks": st.blocks,
                "shards": [{k: getattr(st.shard[g], k) for k, _ in _NodeShardStats._fields_} for g in range(st.nshards)]}

    def run_digest(self, ch):
        """gpsbb_node_run_digest: the driver's own sink — one 64-bit digest per block, taken on the GPU that rendered it by the
        shard's producer thread (no Python in the data path); returns (statistics, uint64 [nblocks])"""
        ch = _as_chan(ch)
        if ch.ndim != 2 or ch.shape[1] != self.nch:
            raise ValueError("descriptors of shape (nblocks, %d) wanted, got %r" % (self.nch, ch.shape))
        digs = np.zeros(ch.shape[0], np.uint64)
        st = _NodeStats()
        _chk(lib().gpsbb_node_run_digest(self._n, ch.ctypes.data, ch.shape[0], digs.ctypes.data, C.byref(st)), "gpsbb_node_run_digest")
        return {"rc": 0, "seconds": st.seconds, "blocks": st.blocks,
                "shards": [{k: getattr(st.shard[g], k) for k, _ in _NodeShardStats._fields_} for g in range(st.nshards)]}, digs

    def slot_digests(self, shard, nblocks):
        """gpsbb_node_slot_digests, from inside a sink of a NODE_DIGESTS node: the digests the blocks just handed over were rendered with"""
        out = np.zeros(nblocks, np.uint64)
        _chk(lib().gpsbb_node_slot_digests(self._n, shard, out.ctypes.data, nblocks), "gpsbb_node_slot_digests")
        return out

    def begin(self, sink):
        """gpsbb_node_begin: an incremental run; feed() the stream as it comes, end() when it is over"""
        self._raised = []

        def guarded(user, iq, first, nb, shard):
            try:
                return int(sink(iq, first, nb, shard) or 0)
            except BaseException as e:  # noqa: BLE001
                self._raised.append(e)
                return -1
        self._cb = NODE_SINK(guarded)
        _chk(lib().gpsbb_node_begin(self._n, C.cast(self._cb, C.c_void_p), None), "gpsbb_node_begin")

    def feed(self, ch):
        ch = _as_chan(ch)
        if ch.ndim != 2 or ch.shape[1] != self.nch:
            raise ValueError("descriptors of shape (nblocks, %d) wanted, got %r" % (self.nch, ch.shape))
        _chk(lib().gpsbb_node_feed(self._n, ch.ctypes.data, ch.shape[0]), "gpsbb_node_feed")

    def end(self, expect_stop=False):
        st = _NodeStats()
        rc = lib().gpsbb_node_end(self._n, C.byref(st))
        self._cb = None
        if self._raised:
            raise self._raised[0]
        if rc != 0 and not (expect_stop and rc == -7):
            raise GpsbbError(rc, "gpsbb_node_end")
        return {"rc": rc, "seconds": st.seconds, "blocks": st.blocks,
                "shards": [{k: getattr(st.shard[g], k) for k, _ in _NodeShardStats._fields_} for g in range(st.nshards)]}


def out_bytes(fmt, nsamp):
    """gpsbb_out_bytes: bytes of one block of nsamp samples in output format fmt (GpsbbError for a format it refuses)"""
    n = lib().gpsbb_out_bytes(fmt, nsamp)
    _chk(n if n < 0 else 0, "gpsbb_out_bytes")
    return n


def _out_layout(nblocks, nsamp, fmt):
    f = (fmt & OUT_FORMAT_MASK) >> 8
    return {0: (np.int16, C.c_int16, (nblocks, nsamp, 2)), 1: (np.int8, C.c_int8, (nblocks, nsamp, 2)),
            2: (np.uint8, C.c_uint8, (nblocks, nsamp // 4))}[f]


def iq_view(ptr, nblocks, nsamp, fmt=OUT_SC16):
    """A numpy view of nblocks blocks in output format fmt at host address ptr (a popped slot, a node sink's iq): int16
    [nblocks, nsamp, 2] (SC16), int8 [nblocks, nsamp, 2] (SC8), uint8 [nblocks, nsamp // 4] (SC1)"""
    _, ct, shape = _out_layout(nblocks, nsamp, fmt)
    return np.ctypeslib.as_array(C.cast(C.c_void_p(ptr), C.POINTER(ct)), shape)


def _as_out(buf, nblocks, nsamp, fmt):
    """iq_view's shape over a numpy buffer (a view of it: the buffer stays alive)"""
    dt, _, shape = _out_layout(nblocks, nsamp, fmt)
    n = nblocks * out_bytes(fmt, nsamp)
    return buf.reshape(-1).view(np.uint8)[:n].view(dt).reshape(shape)


def pack_iq(iq, fmt):
    """The output formats in numpy (the reference the GPU's packing is checked against): iq int16 [..., nsamp, 2] -> int16 as is
    (SC16), int8 [..., nsamp, 2] (SC8: clamp(v >> shift, -128, 127), an arithmetic shift), uint8 [..., nsamp // 4] (SC1: bit k =
    component k > 0, component 8m in bit 7 of byte m; nsamp % 4 == 0)."""
    a = np.asarray(iq, np.int16)
    if a.ndim < 2 or a.shape[-1] != 2:
        raise ValueError("iq of shape (..., nsamp, 2) wanted, got %r" % (a.shape,))
    f, shift = (fmt & OUT_FORMAT_MASK) >> 8, (fmt & OUT_SHIFT_MASK) >> 12
    if fmt >> 16 or f > 2 or (shift and f != 1):
        raise ValueError("unknown output format 0x%x" % fmt)
    if f == 0:
        return a.copy()
    if f == 1:
        return np.clip(a.astype(np.int32) >> shift, -128, 127).astype(np.int8)
    if a.shape[-2] % 4:
        raise ValueError("1-bit output needs nsamp % 4 == 0")
    bits = (a > 0).reshape(a.shape[:-2] + (a.shape[-2] * 2,))
    return np.packbits(bits, axis=-1, bitorder="big")


def noise_sigma(cn0_dbhz, gain=1.0, delt=1 / 2.6e6):
    """gpsbb_noise_sigma: sigma per component (int16 LSB) of a channel of gain `gain` at C/N0 cn0_dbhz, sample period delt"""
    return lib().gpsbb_noise_sigma(float(cn0_dbhz), float(gain), float(delt))


def noise_table():
    """gpsbb_noise_table: the knots K of the noise's normal deviate, int32 [NOISE_KNOTS] (Q16)"""
    n = lib().gpsbb_noise_table(None, 0)
    k = np.zeros(n, np.int32)
    lib().gpsbb_noise_table(k.ctypes.data, n)
    return k


_PHILOX_M, _PHILOX_W = (0xD2511F53, 0xCD9E8D57), (0x9E3779B9, 0xBB67AE85)


def philox4x32_10(ctr, key):
    """Philox4x32-10 in numpy: ctr uint32-valued [..., 4], key (k0, k1) -> uint32 [..., 4]"""
    c = np.asarray(ctr, np.uint64) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M[0]) * c0, np.uint64(_PHILOX_M[1]) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0), p1 & m32, ((p0 >> s32) ^ c3 ^ k1), p0 & m32
        k0, k1 = (k0 + np.uint64(_PHILOX_W[0])) & m32, (k1 + np.uint64(_PHILOX_W[1])) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _s256(sigma):
    """round(256 * sigma), halves away from zero (llround): 256 * sigma is exact, so is its fraction"""
    x = 256.0 * float(sigma)
    fl = math.floor(x)
    return int(fl) + (1 if x - fl >= 0.5 else 0)


def noise_z(u, table=None):
    """step 2 of the definition: uint32 words -> the Q16 normal deviate z (int64)"""
    K = np.asarray(noise_table() if table is None else table, np.int64)
    u = np.asarray(u, np.uint64)
    t = (np.int64(0x7FFFFFFF) - (u & np.uint64(0x7FFFFFFF)).astype(np.int64))
    e = np.frexp((t | 64).astype(np.float64))[1].astype(np.int64) - 1
    g = e - 6
    r = t & ((np.int64(1) << g) - 1)
    f = np.where(g <= 16, r << np.maximum(16 - g, 0), r >> np.maximum(g - 16, 0))
    i = np.where(t < 64, t, 64 * (e - 5) + ((t >> g) & 63))
    a = K[i] + (((K[np.minimum(i + 1, K.size - 1)] - K[i]) * f + 32768) >> 16)
    return np.where((u >> np.uint64(31)) != 0, -a, a)


def noise_host(seed, sample0, nsamp, sigma, table=None):
    """The noise N of samples sample0 .. sample0 + nsamp - 1 (steps 1-3 of include/gpsbb.h), int32 [nsamp, 2] (I, Q): the
    reference the GPU's noise is checked against"""
    s = np.uint64(int(sample0)) + np.arange(int(nsamp), dtype=np.uint64)
    m = s >> np.uint64(1)
    m0 = int(m[0]) if nsamp else 0
    mm = np.arange(m0, (int(m[-1]) + 1) if nsamp else m0, dtype=np.uint64)
    ctr = np.zeros(mm.shape + (4,), np.uint64)
    ctr[:, 0] = mm & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = mm >> np.uint64(32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    row = (m - np.uint64(m0)).astype(np.int64)
    col = 2 * (s & np.uint64(1)).astype(np.int64)
    u = np.stack([x[row, col], x[row, col + 1]], axis=-1)
    z = noise_z(u, table)
    return ((np.int64(_s256(sigma)) * z + (1 << 23)) >> 24).astype(np.int32)


def apply_noise(iq, seed, sample0, sigma, shift, table=None):
    """Steps 1-4 in numpy: iq int16 [..., nsamp, 2] (consecutive blocks: one stream from sample0) -> (int16 of iq's shape,
    components saturated): w = sat16((v + N) >> shift), what pack_iq then packs"""
    a = np.asarray(iq, np.int16)
    if a.ndim < 2 or a.shape[-1] != 2:
        raise ValueError("iq of shape (..., nsamp, 2) wanted, got %r" % (a.shape,))
    if not 0 <= int(shift) <= 7:
        raise ValueError("noise shift outside 0..7")
    flat = a.reshape(-1, 2).astype(np.int64)
    n = noise_host(seed, sample0, flat.shape[0], sigma, table).astype(np.int64)
    s = (flat + n) >> int(shift)
    w = np.clip(s, -32768, 32767)
    return w.astype(np.int16).reshape(a.shape), int(np.count_nonzero(w != s))


# ---- interference (include/gpsbb.h, gpsbb_interf_t): the numpy restatement the GPU's bytes are checked against ----

def interf_make(kind, js_db, f0_hz, f1_hz=0.0, sweep_s=0.0, pulse_period_s=0.0, duty=1.0, delt=1 / 2.6e6):
    """gpsbb_interf_make: an emitter from physical units (J/S in dB against a gain-1.0 channel, Hz, seconds) -> an Interf"""
    e = Interf()
    _chk(lib().gpsbb_interf_make(C.byref(e), int(kind), float(js_db), float(f0_hz), float(f1_hz), float(sweep_s),
                                 float(pulse_period_s), float(duty), float(delt)), "gpsbb_interf_make")
    return e


def interf_eval(interf, s, n):
    """gpsbb_interf_eval: J at samples s .. s + n - 1 by the library's host code -> int32 [n, 2] (I, Q)"""
    js = _as_interf(interf)
    out = np.zeros((int(n), 2), np.int32)
    _chk(lib().gpsbb_interf_eval(C.byref(js), int(s), int(n), out.ctypes.data), "gpsbb_interf_eval")
    return out


def interf_host(interf, s, n):
    """J at samples s .. s + n - 1 straight from the definition, every sample on its own, in numpy uint64 (which wraps mod 2^64
    as the definition asks) -> int32 [n, 2] (I, Q).  s comes from the argument, not from the set."""
    js = _as_interf(interf)
    s, n = int(s), int(n)
    if not 0 <= js.n <= INTERF_MAX or s < 0 or n < 0 or s + n > 1 << 63:
        raise ValueError("emitter count or position range out of bounds")
    M = (1 << 64) - 1
    U = np.uint64
    sin512, cos512 = (t.astype(np.int64) for t in sincos_tables())
    pos = U(s) + np.arange(n, dtype=np.uint64)
    J = np.zeros((n, 2), np.int64)

    def tri(x):  # T(x) = x (x - 1) / 2, the product exact below 2^64 for x < 2^32
        return (x * (x - U(1))) >> U(1)

    with np.errstate(over="ignore"):
        for e in list(js.e)[:js.n]:
            F, R, ph0, G = U(e.step & M), U(e.rate & M), U(e.phase0 & M), np.int64(e.level_q16)
            if e.kind == INTERF_CHIRP:
                P = int(e.sweep)
                phi = U((int(F) * P + int(R) * (P * (P - 1) // 2)) & M)
                k, m = pos // U(P), pos % U(P)
                theta = ph0 + k * phi + F * m + R * tri(m)
            elif e.kind == INTERF_CW:
                theta = ph0 + F * pos
            else:
                raise ValueError("unknown emitter kind %d" % e.kind)
            idx = (theta >> U(55)).astype(np.int64)
            j = np.stack([(G * cos512[idx] + 32768) >> 16, (G * sin512[idx] + 32768) >> 16], axis=-1)
            if e.pulse_period:
                on = ((pos + U(e.pulse_offset)) % U(e.pulse_period)) < U(e.pulse_on)
                j = np.where(on[:, None], j, 0)
            J += j
    return J.astype(np.int32)


def apply_impair(iq, noise, interf):
    """Steps 1-4 with interference in numpy: iq int16 [..., nsamp, 2] (consecutive blocks: one stream from the set's sample0) ->
    (int16 of iq's shape, components saturated): w = sat16((v + N + J) >> shift), N = 0 for noise None"""
    a = np.asarray(iq, np.int16)
    if a.ndim < 2 or a.shape[-1] != 2:
        raise ValueError("iq of shape (..., nsamp, 2) wanted, got %r" % (a.shape,))
    nz, js = _as_noise(noise), _as_interf(interf)
    if not 0 <= js.shift <= 7:
        raise ValueError("shift outside 0..7")
    if nz is not None and (nz.sample0 != js.sample0 or nz.shift != js.shift):
        raise ValueError("noise and interference disagree on sample0 or shift")
    flat = a.reshape(-1, 2).astype(np.int64)
    t = flat + interf_host(js, js.sample0, flat.shape[0]).astype(np.int64)
    if nz is not None:
        t = t + noise_host(nz.seed, nz.sample0, flat.shape[0], nz.sigma).astype(np.int64)
    sft = t >> int(js.shift)
    w = np.clip(sft, -32768, 32767)
    return w.astype(np.int16).reshape(a.shape), int(np.count_nonzero(w != sft))


# ---- output level (include/gpsbb.h, gpsbb_level_t): the numpy restatement the GPU's counts are checked against ----

def level_class(x):
    """m(x): the bit length of x for x >= 0 and of ~x otherwise, for |x| < 2^52 (frexp of the integer as a double is exact)"""
    x = np.asarray(x, np.int64)
    y = np.where(x < 0, ~x, x)
    return np.frexp(y.astype(np.float64))[1].astype(np.int64)


def level_host(iq, noise=None, interf=None):
    """The level of the render iq [nblocks, nsamp, 2] (or [nsamp, 2]: one block; int16, or wider integers with |x| < 2^52 in
    the end, for checks of the classes alone) straight from the definition:
    x = iq + J + N in int64 over one stream from the noise's / the set's sample0, the bit length of every x, a bincount per block
    and component, the sum of x^2 in Python integers -> LEVEL_DTYPE [nblocks].  What the GPU's result equals, field for field."""
    a = np.asarray(iq)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[-1] != 2 or a.dtype.kind not in "iu":
        raise ValueError("integer iq of shape (nblocks, nsamp, 2) wanted, got %s %r" % (a.dtype, a.shape))
    nz, js = _as_noise(noise), _as_interf(interf)
    if nz is not None and js is not None and (nz.sample0 != js.sample0 or nz.shift != js.shift):
        raise ValueError("noise and interference disagree on sample0 or shift")
    nb, nsamp = a.shape[:2]
    x = a.reshape(-1, 2).astype(np.int64)
    if js is not None:
        x = x + interf_host(js, js.sample0, x.shape[0]).astype(np.int64)
    if nz is not None:
        x = x + noise_host(nz.seed, nz.sample0, x.shape[0], nz.sigma).astype(np.int64)
    x = x.reshape(nb, nsamp, 2)
    m = level_class(x)
    out = np.zeros(nb, LEVEL_DTYPE)
    out["n"] = nsamp
    for b in range(nb):
        for c in range(2):
            out["hist"][b, c] = np.bincount(m[b, :, c], minlength=LEVEL_CLASSES)[:LEVEL_CLASSES]
            xc = x[b, :, c]
            hi, lo = xc >> 12, xc & 0xFFF  # x^2 = hi^2 2^24 + 2 hi lo 2^12 + lo^2: every partial sum far below 2^63
            out["sumsq"][b, c] = ((int((hi * hi).sum()) << 24) + (int((hi * lo).sum()) << 13) + int((lo * lo).sum())) & 0xFFFFFFFFFFFFFFFF
    return out


def _as_levels(levels):
    lv = np.ascontiguousarray(levels, dtype=LEVEL_DTYPE).reshape(-1)
    if lv.size < 1:
        raise ValueError("at least one level record wanted")
    return lv


def level_clips(levels, shift, fmt=OUT_SC16):
    """gpsbb_level_clips -> (components step 4 saturates at `shift`, components SC8 then clamps for fmt OUT_SC8(shift8), else 0)"""
    lv = _as_levels(levels)
    c16, c8 = C.c_uint64(), C.c_uint64()
    _chk(lib().gpsbb_level_clips(lv.ctypes.data, lv.size, int(shift), fmt, C.byref(c16), C.byref(c8)), "gpsbb_level_clips")
    return int(c16.value), int(c8.value)


def level_choose(levels, fmt, clip_ppm=100.0):
    """gpsbb_level_choose -> (shift, shift8, met): the smallest shifts whose predicted clips stay within clip_ppm parts per million
    of the components; met is False when even (7, 15) does not"""
    lv = _as_levels(levels)
    a, q = C.c_int(), C.c_int()
    rc = lib().gpsbb_level_choose(lv.ctypes.data, lv.size, fmt, float(clip_ppm), C.byref(a), C.byref(q))
    if rc < 0:
        raise GpsbbError(rc, "gpsbb_level_choose")
    return a.value, q.value, rc == 0


def level_rms(levels, component):
    """gpsbb_level_rms: sqrt(sum sumsq[component] / sum n) over the blocks"""
    lv = _as_levels(levels)
    return lib().gpsbb_level_rms(lv.ctypes.data, lv.size, int(component))


# ---- despreading (include/gpsbb.h, gpsbb_batch_despread): the numpy restatement the GPU's sums are checked against ----

def despread_segments(nsamp, seg_tiles):
    """gpsbb_despread_segments: ceil(nsamp / (1024 * seg_tiles))"""
    n = lib().gpsbb_despread_segments(int(nsamp), int(seg_tiles))
    _chk(n if n < 0 else 0, "gpsbb_despread_segments")
    return n


def cn0_estimate(p, seg_seconds):
    """gpsbb_cn0_estimate over the whole segments p: int64 [n, 2] (P.i, P.q) of one channel, each seg_seconds long -> dB-Hz
    (NaN for n < 2, a zero variance of P.q or a mean of P.i that is not positive)"""
    a = np.ascontiguousarray(p, np.int64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("segments of shape (n, 2) wanted, got %r" % (a.shape,))
    return lib().gpsbb_cn0_estimate(a.ctypes.data, a.shape[0], 1, float(seg_seconds))


def view_host(iq, fmt=OUT_SC16, noise=None, interf=None):
    """What a receiver of output format fmt sees of the int16 render iq [..., nsamp, 2] (consecutive blocks: one stream from
    noise.sample0): apply_noise, then the format's quantiser, unpacked -> int64 of iq's shape (SC16: w; SC8: clamp(w >> shift,
    -128, 127); SC1: +1 where w > 0, else -1; any nsamp).  interf: apply_impair in apply_noise's place"""
    a = np.asarray(iq, np.int16)
    nz = _as_noise(noise)
    if interf is not None:
        a, _ = apply_impair(a, nz, interf)
    elif nz is not None:
        a, _ = apply_noise(a, nz.seed, nz.sample0, nz.sigma, nz.shift)
    f, shift = (fmt & OUT_FORMAT_MASK) >> 8, (fmt & OUT_SHIFT_MASK) >> 12
    if fmt & ~(OUT_FORMAT_MASK | OUT_SHIFT_MASK) or f > 2 or (shift and f != 1):
        raise ValueError("unknown output format 0x%x" % fmt)
    w = a.astype(np.int64)
    if f == 1:
        return np.clip(w >> shift, -128, 127)
    if f == 2:
        return np.where(w > 0, 1, -1).astype(np.int64)
    return w


def despread_host(u, replicas, seg_tiles):
    """The prompt sums in numpy: u [nblocks, nsamp, 2] (uI, uQ: view_host's), replicas [nblocks, nch, nsamp, 2] ((c, s) of every
    channel; zeros for an idle one) -> int64 [nblocks, nch, nseg, 2]: P.i = sum(uI*c + uQ*s), P.q = sum(uQ*c - uI*s) over the
    segments of 1024 * seg_tiles samples (the last one shorter)"""
    u = np.asarray(u, np.int64)
    r = np.asarray(replicas, np.int64)
    if u.ndim != 3 or r.ndim != 4 or u.shape[-1] != 2 or r.shape[-1] != 2 or r.shape[0] != u.shape[0] or r.shape[2] != u.shape[1]:
        raise ValueError("u [nblocks, nsamp, 2] and replicas [nblocks, nch, nsamp, 2] wanted, got %r and %r" % (u.shape, r.shape))
    if seg_tiles < 1:
        raise ValueError("seg_tiles < 1")
    nsamp = u.shape[1]
    seg = 1024 * int(seg_tiles)
    edges = np.arange(0, nsamp, seg)
    out = np.zeros((r.shape[0], r.shape[1], edges.size, 2), np.int64)
    for b in range(r.shape[0]):   # (block by block: the products of a whole batch would be held twice over)
        ui, uq = u[b, None, :, 0], u[b, None, :, 1]
        out[b, :, :, 0] = np.add.reduceat(ui * r[b, :, :, 0] + uq * r[b, :, :, 1], edges, axis=1)
        out[b, :, :, 1] = np.add.reduceat(uq * r[b, :, :, 0] - ui * r[b, :, :, 1], edges, axis=1)
    return out


def despread_lags_host(u, replicas, seg_tiles, lags):
    """gpsbb_batch_despread_lags in numpy: despread_host with the view taken lags[l] samples later than the replica, u padded
    with zeros on either side (a block does not see its neighbours) -> int64 [nblocks, nch, nseg, nlags, 2]"""
    u = np.asarray(u, np.int64)
    lg = [int(v) for v in np.asarray(lags).reshape(-1)]
    if u.ndim != 3 or u.shape[-1] != 2:
        raise ValueError("u [nblocks, nsamp, 2] wanted, got %r" % (u.shape,))
    nsamp = u.shape[1]
    pad = max([abs(v) for v in lg] + [0])
    up = np.zeros((u.shape[0], nsamp + 2 * pad, 2), np.int64)
    up[:, pad:pad + nsamp] = u
    return np.stack([despread_host(up[:, pad + v:pad + v + nsamp], replicas, seg_tiles) for v in lg], axis=3)


def acq_min_shift(view, ncoh, nnc):
    """gpsbb_acq_min_shift: the smallest shift the overflow rule allows"""
    a = lib().gpsbb_acq_min_shift(view, int(ncoh), int(nnc))
    _chk(a if a < 0 else 0, "gpsbb_acq_min_shift")
    return a


def acq_make(delt, f_min_hz, f_step_hz, nbins, coh_s, nlags=0, nnc=1, view=OUT_SC16):
    """gpsbb_acq_make: an AcqCfg from physical units (nlags <= 0: one code period)"""
    cfg = AcqCfg()
    _chk(lib().gpsbb_acq_make(C.byref(cfg), float(delt), float(f_min_hz), float(f_step_hz), int(nbins), float(coh_s), int(nlags), int(nnc),
                              view), "gpsbb_acq_make")
    return cfg


def acq_best(rows, cfg, prn):
    """gpsbb_acq_best: (bin, lag, peak, ratio) of PRN prn's rows"""
    r = np.ascontiguousarray(rows, ACQ_ROW_DTYPE)
    if r.shape != (ACQ_PRNS, cfg.nbins):
        raise ValueError("rows [32, nbins] wanted, got %r" % (r.shape,))
    b, l, pk, ratio = C.c_int(), C.c_int(), C.c_uint64(), C.c_double()
    _chk(lib().gpsbb_acq_best(r.ctypes.data, C.byref(cfg), int(prn), C.byref(b), C.byref(l), C.byref(pk), C.byref(ratio)), "gpsbb_acq_best")
    return b.value, l.value, pk.value, ratio.value


def acq_chips(cfg, prns):
    """the replica of the definition: int64 [len(prns), nnc * ncoh], +1 where chip ((code_step * m) >> 32) mod 1023 is 1, else -1"""
    m = np.arange(int(cfg.nnc) * int(cfg.ncoh), dtype=np.uint64)
    c = ((np.uint64(cfg.code_step) * m) >> np.uint64(32)) % np.uint64(1023)
    return np.stack([2 * codegen(p).astype(np.int64)[c.astype(np.int64)] - 1 for p in prns]) if len(prns) else np.zeros((0, m.size), np.int64)


def acq_mix(u, step):
    """the mixed signal of one bin: u int64 [nsamp, 2] (view_host's) -> (yI, yQ) int64 [nsamp], w * conj(carrier) with the table
    index ((uint32)(step * n)) >> 23"""
    sin512, cos512 = sincos_tables()
    n = np.arange(u.shape[0], dtype=np.uint64)
    idx = (((np.uint64(int(step) & 0xFFFFFFFF) * n) & np.uint64(0xFFFFFFFF)) >> np.uint64(23)).astype(np.int64)
    c, s = cos512.astype(np.int64)[idx], sin512.astype(np.int64)[idx]
    return u[:, 0] * c + u[:, 1] * s, u[:, 1] * c - u[:, 0] * s


def acquire_host(u, cfg, blas=None):
    """gpsbb_device_acquire in numpy: u int64 [nsamp, 2] (view_host's output of the buffer) -> (rows ACQ_ROW_DTYPE [32, nbins], grid
    uint64 [32, nbins, nlags]); PRNs outside cfg.prn_mask are left zero (and cost nothing).  Per bin and interval the coherent
    sums are the chips [PRN, N] times the sliding-window matrix y[m + L] [N, nlags].  blas=False forms them in int64, one PRN at
    a time (np.correlate: the same sums without the matrix); blas=True as one float64 product, which is the same numbers: every
    term and every partial sum, in any order, is an integer below N * Wmax * 1024 <= 2^45 < 2^53.  None: float64 for more than
    four PRNs.  Shift, squares and sums are int64 / uint64 / Python integers either way."""
    u = np.asarray(u, np.int64)
    if u.ndim != 2 or u.shape[1] != 2:
        raise ValueError("u [nsamp, 2] wanted, got %r" % (u.shape,))
    N, P, nnc, a, nbins = int(cfg.ncoh), int(cfg.nlags), int(cfg.nnc), int(cfg.shift), int(cfg.nbins)
    if u.shape[0] < nnc * N + P - 1:
        raise ValueError("nsamp < nnc * ncoh + nlags - 1")
    prns = [p for p in range(1, ACQ_PRNS + 1) if (int(cfg.prn_mask) >> (p - 1)) & 1]
    blas = len(prns) > 4 if blas is None else blas
    x = acq_chips(cfg, prns)
    xm = x.astype(np.float64) if blas else x
    grid = np.zeros((ACQ_PRNS, nbins, P), np.uint64)
    rows = np.zeros((ACQ_PRNS, nbins), ACQ_ROW_DTYPE)
    if not prns:
        return rows, grid
    lc = max(1, min(P, (1 << 23) // max(N, 1)))   # delays per product: the window matrix stays near 64 MB
    pi = np.array(prns) - 1
    for k in range(nbins):
        y = acq_mix(u, cfg.step[k])
        m = np.zeros((len(prns), P), np.uint64)
        for i in range(nnc):
            for l0 in range(0, P, lc if blas else P):
                l1 = min(P, l0 + lc) if blas else P
                for yc in y:
                    seg = yc[i * N + l0:i * N + N + l1 - 1]
                    if blas:
                        w = np.lib.stride_tricks.sliding_window_view(seg, l1 - l0)   # [N, delays]
                        sc = (xm[:, i * N:(i + 1) * N] @ w.astype(np.float64)).astype(np.int64)
                    else:
                        sc = np.stack([np.correlate(seg, xp[i * N:(i + 1) * N], "valid") for xp in xm])
                        assert sc.dtype == np.int64
                    t = (sc >> a).astype(np.uint64)
                    m[:, l0:l1] += t * t
        grid[pi, k] = m
    rows["peak"] = grid.max(axis=2)
    rows["lag"] = grid.argmax(axis=2)
    hi32, lo32 = (grid >> np.uint64(32)).sum(axis=2), (grid & np.uint64(0xFFFFFFFF)).sum(axis=2)   # nlags <= 2^15: below 2^47
    for p in range(ACQ_PRNS):
        for k in range(nbins):
            tot = (int(hi32[p, k]) << 32) + int(lo32[p, k])
            rows["sum_lo"][p, k], rows["sum_hi"][p, k] = tot & 0xFFFFFFFFFFFFFFFF, tot >> 64
    return rows, grid


def trk_make(delt, fll_gain=0.0, pll_bw_hz=0.0, dll_gain=0.0, nfll=0, max_epochs=0):
    """gpsbb_trk_make: a TrkCfg from physical units; an argument <= 0 takes its default (0.15, 15 Hz, 0.1, 100 epochs, 1000 records)"""
    cfg = TrkCfg()
    _chk(lib().gpsbb_trk_make(C.byref(cfg), float(delt), float(fll_gain), float(pll_bw_hz), float(dll_gain), int(nfll), int(max_epochs)),
         "gpsbb_trk_make")
    return cfg


def trk_seed(acq_cfg, prn, bin, lag):
    """gpsbb_trk_seed: a channel's first state (TRK_STATE_DTYPE, one element) from an acquisition hit"""
    st = np.zeros(1, TRK_STATE_DTYPE)
    _chk(lib().gpsbb_trk_seed(st.ctypes.data, C.byref(acq_cfg), int(prn), int(bin), int(lag)), "gpsbb_trk_seed")
    return st[0]


def trk_bitsync(epochs, skip):
    """gpsbb_trk_bitsync -> (offset, hist int32 [20]): the sign changes of p_i after record `skip`, by record index mod 20"""
    e = np.ascontiguousarray(epochs, TRK_EPOCH_DTYPE).reshape(-1)
    off, hist = C.c_int(), np.zeros(20, np.int32)
    _chk(lib().gpsbb_trk_bitsync(e.ctypes.data, e.size, int(skip), C.byref(off), hist.ctypes.data), "gpsbb_trk_bitsync")
    return off.value, hist


def trk_bits(epochs, first, max_bits=None):
    """gpsbb_trk_bits -> int8 [nbits]: the signs of the sums of p_i over whole groups of 20 records from record `first`"""
    e = np.ascontiguousarray(epochs, TRK_EPOCH_DTYPE).reshape(-1)
    cap = e.size // 20 + 1 if max_bits is None else int(max_bits)
    bits = np.zeros(max(cap, 1), np.int8)
    n = lib().gpsbb_trk_bits(e.ctypes.data, e.size, int(first), bits.ctypes.data, cap)
    _chk(n if n < 0 else 0, "gpsbb_trk_bits")
    return bits[:n].copy()


def _tdiv(a, b):
    """C's / on integers: truncates toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _trk_m(x):
    """m(x): the bit length of x for x >= 0, of ~x otherwise"""
    return (x if x >= 0 else ~x).bit_length()


def _clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def trk_plan_host(cfg, st):
    """steps 1 and 2 of an epoch in Python integers: st a dict of a state's fields -> (cs, N)"""
    nom = int(cfg.code_nom)
    aid = _tdiv(st["carr_step"], int(cfg.aid_div)) if int(cfg.aid_div) else 0
    cs = _clamp(nom + aid + st["code_adj"], nom - nom // 8, nom + nom // 8)
    return cs, -((st["code_phase"] - TRK_LEN) // cs)


def trk_close_host(cfg, st, cs, N, sums):
    """steps 4 to 8 in Python integers: the six sums (E.i, E.q, P.i, P.q, L.i, L.q) of the epoch correlated at st (a dict of a
    state's fields, advanced in place) with cs and N -> the record, a dict of TRK_EPOCH_DTYPE's fields"""
    cmax = (1 << 47) - 1
    q = max(0, max(_trk_m(v) for v in sums) - 20)
    Ei, Eq, Pi, Pq, Li, Lq = (v >> q for v in sums)
    E2, L2 = Ei * Ei + Eq * Eq, Li * Li + Lq * Lq
    e_d = _tdiv((E2 - L2) << 14, E2 + L2 + 1)
    mode = 0 if st["epoch"] < int(cfg.nfll) else 1
    used = st["carr_step"]
    if mode == 0:
        e_c = 0
        if st["epoch"] > 0:
            cross, dot = st["prev_i"] * Pq - st["prev_q"] * Pi, st["prev_i"] * Pi + st["prev_q"] * Pq
            e_c = _tdiv(((1 if dot >= 0 else -1) * cross) << 14, abs(dot) + abs(cross) + 1)
        st["carr_int"] = _clamp(st["carr_int"] + int(cfg.kf) * e_c, -cmax, cmax)
        st["carr_step"] = st["carr_int"]
    else:
        e_c = _tdiv(((1 if Pi >= 0 else -1) * Pq) << 14, abs(Pi) + abs(Pq) + 1)
        st["carr_int"] = _clamp(st["carr_int"] + int(cfg.kp2) * e_c, -cmax, cmax)
        st["carr_step"] = _clamp(st["carr_int"] + int(cfg.kp1) * e_c, -cmax, cmax)
    st["code_int"] = _clamp(st["code_int"] + int(cfg.kd2) * e_d, -(1 << 56), 1 << 56)
    st["code_adj"] = (st["code_int"] + int(cfg.kd1) * e_d) >> 8
    rec = dict(n0=st["n0"], N=N, q=q, e_i=sums[0], e_q=sums[1], p_i=sums[2], p_q=sums[3], l_i=sums[4], l_q=sums[5], carr_step=used,
               code_phase=st["code_phase"], carr_phase=st["carr_phase"], e_c=e_c, e_d=e_d, mode=mode)
    s32 = (used >> 16) & 0xFFFFFFFF
    st["carr_phase"] = (st["carr_phase"] + s32 * N) & 0xFFFFFFFF
    st["code_phase"] = st["code_phase"] + cs * N - TRK_LEN
    st["n0"] += N
    st["epoch"] += 1
    st["prev_i"], st["prev_q"] = Pi, Pq
    return rec


def track_host(u, cfg, states):
    """gpsbb_device_track in numpy: u int64 [nsamp, 2] (view_host's output of the buffer), states TRK_STATE_DTYPE [nch] (left as
    they are) -> (the states after; per channel its records, a list of TRK_EPOCH_DTYPE arrays).  An epoch's samples are taken at
    once (step 3 vectorised: every product and partial sum an integer below 2^45); steps 1-2 and 4-8 are Python integers."""
    u = np.asarray(u, np.int64)
    if u.ndim != 2 or u.shape[1] != 2:
        raise ValueError("u [nsamp, 2] wanted, got %r" % (u.shape,))
    nsamp = u.shape[0]
    sin512, cos512 = sincos_tables()
    cosv, sinv = cos512.astype(np.int64), sin512.astype(np.int64)
    out_st = np.array(states, TRK_STATE_DTYPE).reshape(-1)
    recs = []
    sp = int(cfg.spacing)
    for c in range(out_st.size):
        st = {k: int(out_st[c][k]) for k in TRK_STATE_DTYPE.names}
        x = 2 * codegen(st["prn"]).astype(np.int64) - 1
        mine = []
        while len(mine) < int(cfg.max_epochs):
            cs, N = trk_plan_host(cfg, st)
            if st["n0"] + N > nsamp:
                break
            j = np.arange(N, dtype=np.uint64)
            s32 = (st["carr_step"] >> 16) & 0xFFFFFFFF
            idx = (((np.uint64(st["carr_phase"]) + np.uint64(s32) * j) & np.uint64(0xFFFFFFFF)) >> np.uint64(23)).astype(np.int64)
            w = u[st["n0"]:st["n0"] + N]
            cc, ss = cosv[idx], sinv[idx]
            yi, yq = w[:, 0] * cc + w[:, 1] * ss, w[:, 1] * cc - w[:, 0] * ss
            phi = np.uint64(st["code_phase"]) + np.uint64(cs) * j   # < LEN
            sums = []
            for o in (sp, 0, -sp):
                chip = ((phi + np.uint64(o + TRK_LEN)) % np.uint64(TRK_LEN)) >> np.uint64(32)
                xs = x[chip.astype(np.int64)]
                sums += [int((xs * yi).sum()), int((xs * yq).sum())]
            mine.append(trk_close_host(cfg, st, cs, N, sums))
        for k in TRK_STATE_DTYPE.names:
            out_st[c][k] = st[k]
        r = np.zeros(len(mine), TRK_EPOCH_DTYPE)
        for i, m in enumerate(mine):
            for k, v in m.items():
                r[i][k] = v
        recs.append(r)
    return out_st, recs


# ---- the front-end filter (include/gpsbb.h, gpsbb_device_fir): the numpy restatement the GPU's output is checked against ----

def fir_make(ntaps, decim, cutoff=0.0, atten_db=0.0):
    """gpsbb_fir_make: a Kaiser-windowed sinc for decimation by decim -> Fir (cutoff: a fraction of the output's Nyquist rate,
    default 0.8; atten_db: default 60)"""
    f = Fir()
    _chk(lib().gpsbb_fir_make(C.byref(f), int(ntaps), int(decim), float(cutoff), float(atten_db)), "gpsbb_fir_make")
    return f


def fir_host(w, fir, hist=None):
    """gpsbb_device_fir in numpy on view samples w [nsamp, 2] (view_host's output: already impaired) -> (y int16 [nsamp / D, 2],
    the history to hand on int16 [T - 1, 2], the components the clamp changed).  hist: [T - 1, 2] or None (zeros)"""
    T, D, shift = int(fir.ntaps), int(fir.decim), int(fir.shift)
    h = fir.taps()
    w = np.asarray(w, np.int64)
    if not (1 <= T <= FIR_MAX_TAPS and 1 <= D <= FIR_MAX_DECIM and 0 <= shift <= FIR_MAX_SHIFT and int(np.abs(h).sum()) <= FIR_MAX_SUM):
        raise ValueError("a filter gpsbb_device_fir refuses")
    if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] < 1 or w.shape[0] % D:
        raise ValueError("w of shape (nsamp, 2) with nsamp a multiple of %d wanted, got %r" % (D, w.shape))
    hin = np.zeros((T - 1, 2), np.int64) if hist is None else np.asarray(hist, np.int64).reshape(T - 1, 2)
    x = np.concatenate([hin, w])              # x[T - 1 + n] = w[n]
    M = w.shape[0] // D
    acc = np.zeros((M, 2), np.int64)
    first = T - 1 + D - 1                     # output m, tap k: x[first + m * D - k]
    for k in range(T):
        acc += int(h[k]) * x[first - k: first - k + (M - 1) * D + 1: D]
    y = (acc + (1 << (shift - 1))) >> shift if shift else acc
    out = np.clip(y, -32768, 32767)
    return out.astype(np.int16), x[x.shape[0] - (T - 1):].astype(np.int16), int(np.count_nonzero(out != y))


# ---- the power spectrum (include/gpsbb.h, gpsbb_device_psd): the numpy restatement the GPU's output is checked against ----

def psd_make(log2n, nsamp, hop=0, window=PSD_RECT):
    """gpsbb_psd_make: the plan for nsamp samples -> Psd (hop 0: N for the rectangular window, N / 2 for Hann; the smallest legal shift)"""
    p = Psd()
    _chk(lib().gpsbb_psd_make(C.byref(p), int(log2n), int(hop), int(window), int(nsamp)), "gpsbb_psd_make")
    return p


def psd_min_shift(nseg):
    """gpsbb_psd_min_shift: the smallest shift the overflow rule allows nseg segments"""
    rc = lib().gpsbb_psd_min_shift(int(nseg))
    if rc < 0:
        raise GpsbbError(rc, "gpsbb_psd_min_shift")
    return rc


_psd_tw = None


def psd_twiddles():
    """gpsbb_psd_twiddles -> (c int64 [2048], s int64 [2048]): the library's own table, fetched once"""
    global _psd_tw
    if _psd_tw is None:
        c, s = np.zeros(2048, np.int32), np.zeros(2048, np.int32)
        _chk(lib().gpsbb_psd_twiddles(c.ctypes.data, s.ctypes.data), "gpsbb_psd_twiddles")
        _psd_tw = (c.astype(np.int64), s.astype(np.int64))
    return _psd_tw


def psd_scale(psd, nseg, view=OUT_SC16):
    """gpsbb_psd_scale: the factor from psd[k] to mean square per bin in the view's units (NaN for arguments it refuses)"""
    return float(lib().gpsbb_psd_scale(C.byref(psd), int(nseg), view))


def psd_nseg(psd, nsamp):
    """the segments of nsamp samples under the plan, 0 where none fits"""
    N = 1 << int(psd.log2n)
    return (int(nsamp) - N) // int(psd.hop) + 1 if nsamp >= N and psd.hop >= 1 else 0


def psd_wbits(view):
    return (15, 7, 0)[(view & OUT_FORMAT_MASK) >> 8]


def psd_transform(x):
    """the definition's transform of x int64 [nseg, N, 2] (loaded: windowed, scaled, halved) -> X int64 [nseg, N, 2], a stage at a time"""
    tc, ts = psd_twiddles()
    nseg, N = x.shape[0], x.shape[1]
    L = N.bit_length() - 1
    rev = np.zeros(N, np.int64)
    for b in range(L):
        rev |= ((np.arange(N) >> b) & 1) << (L - 1 - b)
    a = np.empty_like(x)
    a[:, rev] = x
    m = 2
    while m <= N:
        h = m // 2
        k = np.arange(h) * (4096 // m)
        c, s = tc[k], ts[k]
        a = a.reshape(nseg, N // m, m, 2)
        u, v = a[:, :, :h], a[:, :, h:]
        t = np.stack([(v[..., 0] * c + v[..., 1] * s + (1 << 29)) >> 30, (v[..., 1] * c - v[..., 0] * s + (1 << 29)) >> 30], -1)
        a = np.concatenate([(u + t + 1) >> 1, (u - t + 1) >> 1], 2).reshape(nseg, N, 2)
        m *= 2
    return a


def psd_host(w, psd, view=OUT_SC16):
    """gpsbb_device_psd in numpy on view samples w [nsamp, 2] (view_host's output for `view`: impaired and quantised) ->
    (uint64 [N], the segments)"""
    L, hop, shift = int(psd.log2n), int(psd.hop), int(psd.shift)
    w = np.asarray(w, np.int64)
    if not (PSD_MIN_LOG2N <= L <= PSD_MAX_LOG2N and 1 <= hop <= PSD_MAX_HOP and 0 <= shift <= PSD_MAX_SHIFT):
        raise ValueError("a plan gpsbb_device_psd refuses")
    N = 1 << L
    if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] < N:
        raise ValueError("w of shape (nsamp, 2) with nsamp >= %d wanted, got %r" % (N, w.shape))
    nseg = (w.shape[0] - N) // hop + 1
    if nseg > PSD_MAX_NSEG or nseg * 2 * (((1 << 30) >> shift) + 1) ** 2 >= 1 << 64:
        raise ValueError("a plan gpsbb_device_psd refuses: %d segments at shift %d" % (nseg, shift))
    win = psd.window()
    out = np.zeros(N, np.uint64)
    step = max(1, (1 << 16) // N)   # segments at a time: a few MB of int64
    for s0 in range(0, nseg, step):
        idx = (np.arange(s0, min(nseg, s0 + step))[:, None] * hop + np.arange(N)[None, :])
        x = (w[idx] * win[None, :, None] * (1 << (15 - psd_wbits(view)))) >> 1
        X = psd_transform(x) >> shift
        out += (X * X).sum(-1).sum(0).astype(np.uint64)
    return out, nseg


# ---- pulse blanking (include/gpsbb.h, gpsbb_device_blank): the numpy restatement the GPU's output is checked against ----

def blank_make(win=0, pre=-1, hold=-1, floor_ms=0.0, thr_db=0.0):
    """gpsbb_blank_make: the plan from a quiet floor (the mean of |w|^2); the defaults are the call's: L = 8, G = hold = L, 6 dB"""
    b = Blank()
    _chk(lib().gpsbb_blank_make(C.byref(b), int(win), int(pre), int(hold), float(floor_ms), float(thr_db)), "gpsbb_blank_make")
    return b


def blank_from_level(blank, levels, shift=0, thr_db=6.0):
    """gpsbb_blank_from_level: a copy of blank with thr set thr_db above the lower median of the short blocks' levels (LEVEL_DTYPE
    [n], device_level's or level_host's, measured before the shift)"""
    b = blank.copy()
    lv = _as_levels(levels)
    _chk(lib().gpsbb_blank_from_level(C.byref(b), lv.ctypes.data, lv.size, int(shift), float(thr_db)), "gpsbb_blank_from_level")
    return b


def blank_ok(blank):
    """what gpsbb_device_blank asks of a plan"""
    return (1 <= int(blank.win) <= BLANK_MAX_WIN and 0 <= int(blank.pre) <= BLANK_MAX_PRE and 0 <= int(blank.hold) <= BLANK_MAX_HOLD
            and int(blank._pad) == 0)


def blank_host(w, blank, hist=None):
    """gpsbb_device_blank in numpy on view samples w [nsamp, 2] (view_host's output: already impaired) -> (out int16 [nsamp, 2],
    hist_out int16 [K, 2], blanked, triggers), from the definition in include/gpsbb.h: the boxcar is a difference of two prefix
    sums of the powers, the dilation a difference of two prefix counts of the triggers"""
    if not blank_ok(blank):
        raise ValueError("a plan gpsbb_device_blank refuses")
    w = np.asarray(w, np.int64)
    if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] < 1:
        raise ValueError("w of shape (nsamp >= 1, 2) wanted, got %r" % (w.shape,))
    L, G, D, K, thr, n = int(blank.win), int(blank.pre), int(blank.pre) + int(blank.hold), blank.hist(), int(blank.thr), w.shape[0]
    h = np.zeros((K, 2), np.int64) if hist is None else np.asarray(hist, np.int64).reshape(K, 2)
    x = np.concatenate([h, w])                                   # x[K + n'] is w[n'], n' in [-K, nsamp)
    cp = np.concatenate([[0], np.cumsum((x * x).sum(1))])        # cp[i]: the powers before x[i]; below 2^31 * 2^31
    j = np.arange(-D, n)                                         # s[j] = p[j - L + 1] + .. + p[j]
    s = cp[j + K + 1] - cp[j + K + 1 - L]
    trig = s.astype(np.uint64) > np.uint64(thr)
    ct = np.concatenate([[0], np.cumsum(trig)])                  # ct[i]: the triggers before j = i - D
    m = np.arange(n)
    z = ct[m + D + 1] - ct[m] > 0                                # any trig[j], j in [m - D, m]
    out = np.where(z[:, None], 0, x[m + K - G])
    return out.astype(np.int16), x[x.shape[0] - K:].astype(np.int16), int(np.count_nonzero(z)), int(np.count_nonzero(trig[D:]))


def blank_plain_c(w, blank, hist=None):
    """csrc/gpsbb_blank.h's plain-C definition (blank_host, through the experiments build's hook gpsbb_test_blank_host) on host
    memory -> (out, hist_out, blanked, triggers)"""
    w = np.ascontiguousarray(w, np.int16)
    K = min(max(blank.hist(), 0), BLANK_MAX_HIST)
    hin = None if hist is None else np.ascontiguousarray(hist, np.int16).reshape(K, 2)
    out, hout = np.zeros(w.shape, np.int16), np.zeros((K, 2), np.int16)
    blanked, triggers = C.c_uint64(0), C.c_uint64(0)
    _chk(exp_lib().gpsbb_test_blank_host(C.byref(blank), w.ctypes.data, w.shape[0], None if hin is None or K == 0 else hin.ctypes.data, out.ctypes.data,
                                         hout.ctypes.data if K else None, C.byref(blanked), C.byref(triggers)), "gpsbb_test_blank_host")
    return out, hout, int(blanked.value), int(triggers.value)


def blank_tile():
    """(the outputs of one of k_blank's tiles, the tiles of a workgroup's least run): gpsbb_test_blank_tile"""
    run = C.c_int(0)
    t = exp_lib().gpsbb_test_blank_tile(C.byref(run))
    return int(t), int(run.value)


# ---- interference excision (include/gpsbb.h, gpsbb_device_excise): the numpy restatement the GPU's output is checked against ----

def exc_make(log2n):
    """gpsbb_exc_make: the plan with the periodic Hann window, an empty mask and no threshold -> Exc"""
    e = Exc()
    _chk(lib().gpsbb_exc_make(C.byref(e), int(log2n)), "gpsbb_exc_make")
    return e


def exc_from_psd(exc, psd, plan, nseg, mask_db=0.0, thr_db=0.0):
    """gpsbb_exc_from_psd: a copy of exc with the mask (bins more than mask_db above the median of psd) and the threshold (thr_db
    above the median, in a single segment's units) from a spectrum device_psd or psd_host made at SC16 under plan"""
    e = exc.copy()
    p = np.ascontiguousarray(psd, np.uint64)
    if p.size != 1 << min(max(int(exc.log2n), 0), EXC_MAX_LOG2N):
        raise ValueError("a spectrum of the plan's N bins wanted")
    _chk(lib().gpsbb_exc_from_psd(C.byref(e), p.ctypes.data, C.byref(plan), int(nseg), float(mask_db), float(thr_db)), "gpsbb_exc_from_psd")
    return e


def exc_inverse(z, shadow=None):
    """the definition's inverse transform of Z int64 [nseg, N, 2] (natural bin order) -> y int64 [nseg, N, 2], a stage at a time.
    shadow: a list that takes the largest |component| after every stage"""
    tc, ts = psd_twiddles()
    nseg, N = z.shape[0], z.shape[1]
    L = N.bit_length() - 1
    rev = np.zeros(N, np.int64)
    for b in range(L):
        rev |= ((np.arange(N) >> b) & 1) << (L - 1 - b)
    a = np.empty_like(z)
    a[:, rev] = z
    m = 2
    while m <= N:
        h = m // 2
        k = np.arange(h) * (4096 // m)
        c, s = tc[k], ts[k]
        a = a.reshape(nseg, N // m, m, 2)
        u, v = a[:, :, :h], a[:, :, h:]
        t = np.stack([(v[..., 0] * c - v[..., 1] * s + (1 << 29)) >> 30, (v[..., 1] * c + v[..., 0] * s + (1 << 29)) >> 30], -1)
        a = np.concatenate([u + t, u - t], 2).reshape(nseg, N, 2)
        if shadow is not None:
            shadow.append(int(np.abs(a).max()) if a.size else 0)
        m *= 2
    return a


def exc_ok(exc):
    """what gpsbb_device_excise asks of a plan"""
    L = int(exc.log2n)
    if not EXC_MIN_LOG2N <= L <= EXC_MAX_LOG2N:
        return False
    w, H = exc.window(), 1 << (L - 1)
    return bool((w[:H] >= 0).all() and (w[:H] <= EXC_WIN_ONE).all() and (w[:H] + w[H:] == EXC_WIN_ONE).all())


def excise_host(w, exc, hist=None, shadow=None, cells=None):
    """gpsbb_device_excise in numpy on view samples w [nsamp, 2] (view_host's output: already impaired) -> (out int16 [nsamp, 2],
    the history to hand on int16 [N, 2], the components the clamp changed, the (segment, bin) pairs zeroed).  hist: [N, 2] or
    None (zeros).  shadow: a list that takes the largest |component| of every inverse stage (int64: nothing wraps here); cells: a
    list that takes the zeroed cells, bool [nsamp / H + 1, N]"""
    if not exc_ok(exc):
        raise ValueError("a plan gpsbb_device_excise refuses")
    L, thr = int(exc.log2n), int(exc.thr)
    N, H, G = 1 << L, 1 << (L - 1), (L + 1) // 2
    S = 13 - G
    w = np.asarray(w, np.int64)
    if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] < H or w.shape[0] % H:
        raise ValueError("w of shape (nsamp, 2) with nsamp a multiple of %d wanted, got %r" % (H, w.shape))
    nblk = w.shape[0] // H
    hin = np.zeros((N, 2), np.int64) if hist is None else np.asarray(hist, np.int64).reshape(N, 2)
    x = np.concatenate([hin, w])              # x[N + n] = w[n]; segment s covers x[s H .. s H + N)
    win, masked = exc.window(), exc.bins()
    y = np.empty((nblk + 1, N, 2), np.int64)
    excised = 0
    step = max(1, (1 << 16) // N)             # segments at a time: a few MB of int64
    for s0 in range(0, nblk + 1, step):
        sg = np.arange(s0, min(nblk + 1, s0 + step))
        X = psd_transform((x[sg[:, None] * H + np.arange(N)[None, :]] * win[None, :, None]) >> 1)
        pw = (X * X).sum(-1)                  # < 2^62
        zero = masked[None, :] | ((pw > thr) if 0 < thr < 1 << 62 else np.zeros(pw.shape, bool))
        excised += int(np.count_nonzero(zero[sg >= 1]))
        if cells is not None:
            cells.append(zero)
        Z = np.sign(X) * ((np.abs(X) + (1 << (G - 1))) >> G)
        Z[zero] = 0
        y[sg] = exc_inverse(Z, shadow)
    o = (y[:-1, H:] + y[1:, :H] + (1 << (S - 1))) >> S
    out = np.clip(o, -32768, 32767)
    return (out.reshape(nblk * H, 2).astype(np.int16), x[x.shape[0] - N:].astype(np.int16), int(np.count_nonzero(out != o)), excised)


def excise_plain_c(w, exc, hist=None):
    """csrc/gpsbb_exc.h's plain-C definition (exc_host, through the experiments build's hook gpsbb_test_exc_host) on host memory ->
    (out, hist_out, clipped, excised, the largest |component| any inverse step produced)"""
    w = np.ascontiguousarray(w, np.int16)
    N = 1 << min(max(int(exc.log2n), 0), EXC_MAX_LOG2N)
    hin = None if hist is None else np.ascontiguousarray(hist, np.int16).reshape(N, 2)
    out, hout = np.zeros_like(w), np.zeros((N, 2), np.int16)
    clipped, excised, peak = C.c_uint64(0), C.c_uint64(0), C.c_int64(0)
    _chk(exp_lib().gpsbb_test_exc_host(C.byref(exc), w.ctypes.data, w.shape[0], None if hin is None else hin.ctypes.data, out.ctypes.data,
                                       hout.ctypes.data, C.byref(clipped), C.byref(excised), C.byref(peak)), "gpsbb_test_exc_host")
    return out, hout, int(clipped.value), int(excised.value), int(peak.value)


def block_digest_host(iq):
    """gpsbb_device_digest's number for blocks in host memory: iq int16 [..., nsamp, 2] -> uint64 [...]"""
    a = np.ascontiguousarray(iq, np.int16)
    w = a.view(np.uint32).reshape(a.shape[:-2] + (a.shape[-2],)).astype(np.uint64)
    with np.errstate(over="ignore"):
        m = (np.arange(a.shape[-2], dtype=np.uint64) * np.uint64(0x9E3779BA) + np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
        return (w * m).sum(axis=-1, dtype=np.uint64)


class SplitMix64:
    """Counter-mode splitmix64: draw k (k = 1, 2, ...) is mix(seed + k*0x9E3779B97F4A7C15) — the sequence
    the scalar generator produces, evaluated vectorised."""

    def __init__(self, seed):
        self.seed = np.uint64(seed)
        self.k = 0

    def take_at(self, start, n):
        """draws start+1 .. start+n of the sequence (counter mode: any slice costs what it holds)"""
        with np.errstate(over="ignore"):
            idx = np.arange(start + 1, start + n + 1, dtype=np.uint64)
            z = self.seed + idx * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        return z

    def take(self, n):
        z = self.take_at(self.k, n)
        self.k += n
        return z

    def u01(self, shape):
        n = int(np.prod(shape))
        return ((self.take(n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)).reshape(shape)

    def u32(self, shape):
        n = int(np.prod(shape))
        return (self.take(n) >> np.uint64(32)).reshape(shape)

    def rows(self, nrows, width, first, count):
        """rows [first, first+count) of the (nrows, width) table the next nrows*width draws fill; the generator moves on
        past the whole table, so that what follows does not depend on which rows were asked for"""
        z = self.take_at(self.k + first * width, count * width).reshape(count, width)
        self.k += nrows * width
        return z


def synth_descriptors(nblocks, nch=16, seed=0x5EED, max_doppler=5000.0, first=0, count=None, fields=None):
    """Seeded descriptor-level constellation: PRN 1..nch, f_carr ~ U(-max,max) Hz, f_code = 1.023e6 +
    f_carr/1540, code_phase ~ U[0,1023), carr_phase ~ U[0,1), gain ~ U(0.30,0.80), random 30-bit nav
    words, iword in [9,58], ibit in 0..29, icode in 0..19.
    first / count: only blocks [first, first+count) of the nblocks-block table — the same rows the whole table has, at
    the cost of those rows (a rank of a time-sharded run builds its own shard only).  fields: only these (the others stay
    zero): what a carrier-chain-only call reads is ("prn", "f_carr", "carr_phase")."""
    count = nblocks - first if count is None else count
    g = SplitMix64(seed)
    ch = np.zeros((count, nch), CHAN_DTYPE)

    def want(f):
        return fields is None or f in fields

    def u01(width=nch):
        return (g.rows(nblocks, width, first, count) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    def skip(width=nch):
        g.k += nblocks * width

    ch["prn"] = np.arange(1, nch + 1, dtype=np.int32)[None, :]
    if want("f_carr") or want("f_code"):
        ch["f_carr"] = (u01() * 2.0 - 1.0) * max_doppler
        ch["f_code"] = 1.023e6 + ch["f_carr"] / 1540.0
    else:
        skip()
    if want("code_phase"):
        ch["code_phase"] = u01() * 1023.0
    else:
        skip()
    if want("carr_phase"):
        ch["carr_phase"] = u01()
    else:
        skip()
    if fields is not None and not (set(fields) - {"prn", "f_carr", "f_code", "code_phase", "carr_phase"}):
        return ch
    ch["gain"] = 0.30 + 0.50 * u01()
    ch["iword"] = 9 + ((g.rows(nblocks, nch, first, count) >> np.uint64(32)) % np.uint64(50)).astype(np.int32)
    ch["ibit"] = ((g.rows(nblocks, nch, first, count) >> np.uint64(32)) % np.uint64(30)).astype(np.int32)
    ch["icode"] = ((g.rows(nblocks, nch, first, count) >> np.uint64(32)) % np.uint64(20)).astype(np.int32)
    ch["dwrd"] = ((g.rows(nblocks, nch * N_DWRD, first, count) >> np.uint64(32)) & np.uint64(0x3FFFFFFF)).astype(np.uint32).reshape(count, nch, N_DWRD)
    return ch


def code_rate_for(sc, fs):
    """An f_code whose individually rounded product with delt = 1 / fs (c:2709) is exactly `sc` chips per sample: searched
    among the doubles next to sc * fs.  None if there is none (not every product is reachable at every rate)."""
    delt = 1.0 / fs
    f = sc * fs
    for _ in range(200):
        p = f * delt
        if p == sc:
            return f
        f = math.nextafter(f, math.inf if p < sc else -math.inf)
    return None


def grazing_descriptors(nblocks, nch, fs, nsamp, offsets, seed=1, max_doppler=5000.0, fixed=False, samples=None, tol=0.25, f_code=None):
    """Adversarial descriptors for the model kernels (k_synth_ev / k_synth_pd): every (block, channel) is aimed so that
    ONE of its NCOs lands within `k` units of 2^-32 of an integer AT a chosen sample n — the reference's own state there,
    not the linear model's: the phase is refined with the exact jump-ahead (gpsbb_nco.h through the experiments build's
    host hooks, CPU only) until 512*carr_phase(n) resp. code_phase(n) is m + k*2^-32 to `tol` units (k may be fractional).  That is
    where floor() of an in-tile model (c:2697 table index, c:2737 chip) can disagree with the reference and where an index
    or chip change falls (almost) exactly on a sample; k runs over `offsets` (both signs: either side of the integer, inside
    and outside the kernels' danger band).  Channel i of block b aims its carrier when (b + i) is even, its code NCO
    otherwise; with `fixed` (the 32-bit accumulator is exact) always the code.  f_code: a code rate (Hz; one, or one per
    channel) in place of 1.023e6 + f_carr / 1540, applied before aiming.  Returns (descriptors, targets)."""
    from fractions import Fraction
    L = exp_lib()
    rng = np.random.default_rng(seed)
    ch = synth_descriptors(nblocks, nch=nch, seed=seed, max_doppler=max_doppler)
    if f_code is not None:
        ch["f_code"] = np.broadcast_to(np.asarray(f_code, np.float64), (nch,))[None, :]
    delt = 1.0 / fs
    unit = Fraction(1, 1 << 32)
    targets = []
    wr = C.c_longlong(0)
    for b in range(nblocks):
        for i in range(nch):
            k = Fraction(float(offsets[(b * nch + i) % len(offsets)]))
            n = int(samples[(b * nch + i) % len(samples)]) if samples is not None else int(rng.integers(1, nsamp))
            n = min(n, nsamp - 1)
            carrier = (b + i) % 2 == 0 and not fixed
            if carrier:
                s = float(ch["f_carr"][b, i]) * delt            # the individually rounded product of c:2741
                want_frac = unit * k                            # 512*phase(n) = integer + k units
                cp = float(ch["carr_phase"][b, i])
                for _ in range(12):
                    got = Fraction(L.gpsbb_test_carr_jump(cp, s, n)) * 512
                    m = round(got)
                    err = (got - m) - want_frac                 # in table-index units
                    if abs(err) <= unit * Fraction(tol):
                        break
                    cp = float((Fraction(cp) - err / 512) % 1)
                ch["carr_phase"][b, i] = cp
                got = Fraction(L.gpsbb_test_carr_jump(cp, s, n)) * 512
                targets.append((b, i, "carr", n, float(k), float((got - round(got)) / unit)))
            else:
                s = float(ch["f_code"][b, i]) * delt            # c:2709
                x = float(ch["code_phase"][b, i])
                for _ in range(12):
                    got = Fraction(L.gpsbb_test_code_jump(x, s, n, C.byref(wr)))
                    m = round(got)
                    err = (got - m) - unit * k
                    if abs(err) <= unit * Fraction(tol):
                        break
                    x = float((Fraction(x) - err) % 1023)
                ch["code_phase"][b, i] = x
                got = Fraction(L.gpsbb_test_code_jump(x, s, n, C.byref(wr)))
                targets.append((b, i, "code", n, float(k), float((got - round(got)) / unit)))
    if fixed:
        ch["carr_phase"] = np.floor(ch["carr_phase"] * 2.0 ** 32)
    return ch, targets


# ---- time sharding (one process per GPU, no data-path collective) ------------------------------------

def shard_blocks(nblocks, rank, world):
    """Contiguous block range [b0, b1) of rank `rank` out of `world` (BASELINE configs[4]: GPU g gets blocks
    [g*B/G, (g+1)*B/G))."""
    return (nblocks * rank) // world, (nblocks * (rank + 1)) // world


def shard_descriptors(ch, rank, world, delt, nsamp, nthreads=0):
    """Descriptors of this rank's time shard with the exact carrier phase seeded at every block start, so
    the shard can be synthesised without the preceding blocks (gpsbb_chain_carrier_host)."""
    ch = _as_chan(ch).copy()
    ch["carr_phase"] = chain_carrier_host(ch, delt, nsamp, nthreads)
    b0, b1 = shard_blocks(ch.shape[0], rank, world)
    return ch[b0:b1]


# ---- host front end (include/gpsfe.h): RINEX-2 + position/motion -> per-block descriptors -------------

FE_LIB_PATH = os.path.join(HERE, "libgpsfe.so")
_fe_lib = None


class _FeConfig(C.Structure):
    _fields_ = [("navfile", C.c_char_p), ("rinex3", C.c_int), ("motion_file", C.c_char_p), ("use_ecef", C.c_int),
                ("pos", C.c_double * 3), ("have_start", C.c_int), ("y", C.c_int), ("m", C.c_int),
                ("d", C.c_int), ("hh", C.c_int), ("mm", C.c_int), ("sec", C.c_double),
                ("time_overwrite", C.c_int), ("iono_disable", C.c_int), ("max_chan", C.c_int),
                ("fixed_carrier", C.c_int)]


class Echo(C.Structure):
    """gpsfe_echo_t: one multipath echo of satellite prn (include/gpsfe.h)"""
    _fields_ = [("prn", C.c_int), ("extra_m", C.c_double), ("rate_mps", C.c_double), ("atten_db", C.c_double),
                ("phase_cyc", C.c_double)]

    def __init__(self, prn=0, extra_m=0.0, atten_db=0.0, phase_cyc=0.0, rate_mps=0.0):
        super().__init__(int(prn), float(extra_m), float(rate_mps), float(atten_db), float(phase_cyc))


MAX_ECHOES = 8


def build_frontend(force=False):
    hostdir = os.path.join(HERE, "host")
    sim = os.path.join(HERE, "gpsbb-sim")
    newest = max(os.path.getmtime(os.path.join(hostdir, f)) for f in os.listdir(hostdir))
    if force or not os.path.exists(FE_LIB_PATH) or not os.path.exists(sim) or newest > os.path.getmtime(FE_LIB_PATH):
        subprocess.check_call(["make", "-C", hostdir])
    return FE_LIB_PATH


def fe_lib():
    global _fe_lib
    if _fe_lib is None:
        if not os.path.exists(FE_LIB_PATH):
            raise RuntimeError("libgpsfe.so is not built (make -C %s/host)" % HERE)
        L = C.CDLL(FE_LIB_PATH)
        L.gpsfe_open.argtypes = [C.POINTER(_FeConfig), C.POINTER(C.c_void_p)]
        L.gpsfe_close.argtypes = [C.c_void_p]
        L.gpsfe_close.restype = None
        L.gpsfe_strerror.argtypes = [C.c_int]
        L.gpsfe_strerror.restype = C.c_char_p
        L.gpsfe_max_chan.argtypes = [C.c_void_p]
        L.gpsfe_next_block.argtypes = [C.c_void_p, C.c_void_p]
        L.gpsfe_feed_back.argtypes = [C.c_void_p, C.c_void_p]
        L.gpsfe_generate.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.gpsfe_set_threads.argtypes = [C.c_void_p, C.c_int]
        L.gpsfe_time.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.gpsfe_channel_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 4
        L.gpsfe_set_echoes.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.gpsfe_block_chans.argtypes = [C.c_void_p]
        _fe_lib = L
    return _fe_lib


class FrontEnd:
    """gpsfe_open / gpsfe_generate: the scenario the reference's main() runs, as descriptor blocks."""

    def __init__(self, navfile, llh=None, ecef=None, motion=None, start=None, time_overwrite=False,
                 iono=True, max_chan=12, rinex3=False, fixed_carrier=False):
        cfg = _FeConfig()
        cfg.navfile = os.fsencode(navfile)
        cfg.rinex3 = int(rinex3)
        cfg.motion_file = os.fsencode(motion) if motion else None
        if ecef is not None:
            cfg.use_ecef = 1
            cfg.pos = (C.c_double * 3)(*ecef)
        else:
            cfg.pos = (C.c_double * 3)(*(llh if llh is not None else (35.681298, 139.766247, 10.0)))
        if start is not None:  # (y, m, d, hh, mm, sec)
            cfg.have_start = 1
            cfg.y, cfg.m, cfg.d, cfg.hh, cfg.mm = [int(v) for v in start[:5]]
            cfg.sec = float(start[5])
        cfg.time_overwrite = int(time_overwrite)
        cfg.iono_disable = int(not iono)
        cfg.max_chan = max_chan
        cfg.fixed_carrier = int(fixed_carrier)
        self.max_chan = max_chan
        self._fe = C.c_void_p()
        rc = fe_lib().gpsfe_open(C.byref(cfg), C.byref(self._fe))
        if rc != 0:
            raise RuntimeError("gpsfe_open: %s (%d)" % (fe_lib().gpsfe_strerror(rc).decode(), rc))

    def close(self):
        if self._fe:
            fe_lib().gpsfe_close(self._fe)
            self._fe = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_threads(self, n):
        """gpsfe_set_threads: 0 = default (cores up to 16), 1 = the sequential loop"""
        rc = fe_lib().gpsfe_set_threads(self._fe, n)
        if rc != 0:
            raise RuntimeError("gpsfe_set_threads: %d" % rc)

    def set_echoes(self, echoes):
        """gpsfe_set_echoes, before the first block: Echo objects, dicts of Echo's arguments, or tuples in gpsbb-sim -M's
        order (prn, extra_m, atten_db[, phase_cyc[, rate_mps]]); every block has block_chans descriptors afterwards"""
        es = [e if isinstance(e, Echo) else Echo(**e) if isinstance(e, dict) else Echo(*e) for e in echoes]
        arr = (Echo * max(len(es), 1))(*es)
        rc = fe_lib().gpsfe_set_echoes(self._fe, arr, len(es))
        if rc != 0:
            raise RuntimeError("gpsfe_set_echoes: %s (%d)" % (fe_lib().gpsfe_strerror(rc).decode(), rc))

    @property
    def block_chans(self):
        """gpsfe_block_chans: max_chan plus the echoes' slots"""
        return fe_lib().gpsfe_block_chans(self._fe)

    def generate(self, nblocks):
        ch = np.zeros((nblocks, self.block_chans), CHAN_DTYPE)
        rc = fe_lib().gpsfe_generate(self._fe, nblocks, ch.ctypes.data)
        if rc != 0:
            raise RuntimeError("gpsfe_generate: %d" % rc)
        return ch

    def next_block(self):
        ch = np.zeros(self.block_chans, CHAN_DTYPE)
        rc = fe_lib().gpsfe_next_block(self._fe, ch.ctypes.data)
        if rc != 0:
            raise RuntimeError("gpsfe_next_block: %d" % rc)
        return ch

    def feed_back(self, end_state):
        st = np.ascontiguousarray(end_state, dtype=STATE_DTYPE)
        rc = fe_lib().gpsfe_feed_back(self._fe, st.ctypes.data)
        if rc != 0:
            raise RuntimeError("gpsfe_feed_back: %d" % rc)

    def time(self):
        w, s = C.c_int(), C.c_double()
        fe_lib().gpsfe_time(self._fe, C.byref(w), C.byref(s))
        return w.value, s.value
