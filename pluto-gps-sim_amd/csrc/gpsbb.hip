/*
 * gpsbb.hip — host side of libgpsbb: the C ABI of include/gpsbb.h over the HIP kernels in
 * gpsbb_kernels.hip.h.  Plain HIP runtime (streams, events, pinned memory); no torch, no CPU fallback:
 * every fill entry point fails with GPSBB_E_NODEVICE / GPSBB_E_HIP when there is no gfx950 device.
 *
 * Reference interface replaced: the inline sample loop plutogpssim.c:2689-2759 and its producer/consumer
 * contract with pluto_tx_thread_ep (plutogpssim.c:2146-2158).  See include/gpsbb.h.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <chrono>
#include <vector>

#include "gpsbb.h"
#include "gpsbb_kernels.hip.h"
#include "gpsbb_noise.hip.h"
#include "gpsbb_interf.hip.h"
#include "gpsbb_level.hip.h"
#include "gpsbb_events.hip.h"
#include "gpsbb_dense.hip.h"
#include "gpsbb_despread.hip.h"
#include "gpsbb_despread_lags.hip.h"
#include "gpsbb_acq.hip.h"
#include "gpsbb_track.hip.h"
#include "gpsbb_fir.hip.h"
#include "gpsbb_psd.hip.h"
#include "gpsbb_exc.hip.h"
#include "gpsbb_blank.hip.h"
#include "gpsbb_walk.hip.h"
#include "gpsbb_laps.hip.h"
#include "gpsbb_nco.h"
#include "gpsbb_testhooks.h"
#ifdef GPSBB_EXPERIMENTS
#include "gpsbb_modelerr.hip.h"
#endif

using namespace gpsbb_impl;

/* Measurement knobs.  The library as shipped reads NO environment variable: a drop-in must not change its behaviour with
 * what happens to be in its host's environment.  The experiments build (make exp: -DGPSBB_EXPERIMENTS ->
 * libgpsbb_exp.so, which the tuning scripts under tools/ and the NCO unit tests load) turns the constants below into
 * getenv look-ups and exports the gpsbb_test_* hooks. */
#ifdef GPSBB_EXPERIMENTS
#define GPSBB_KNOB_LONG(name, dflt) ([](long d) -> long { static const char *const e = getenv(name); return e ? atol(e) : d; }((long)(dflt)))
#define GPSBB_KNOB_SET(name) ([]() -> bool { static const bool v = getenv(name) != nullptr; return v; }())
#else
#define GPSBB_KNOB_LONG(name, dflt) ((long)(dflt))
#define GPSBB_KNOB_SET(name) (false)
#endif

/* ================================================================================================== */
/* host-side tables                                                                                   */
/* ================================================================================================== */

namespace {

/* sinTable512 / cosTable512 (plutogpssim.c:93-161) from their closed form trunc(511*f(2*pi*i/512)+1.0);
 * guarded by a checksum of the 1024 values so that a libm that rounds differently fails loudly instead
 * of silently changing the output. */
constexpr uint64_t kSinCosFnv1a = 0x1c99a5cf84551314ull;

bool make_sincos(int32_t sin512[512], int32_t cos512[512])
{
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < 512; i++) {
        const double a = two_pi * (double)i / 512.0;
        sin512[i] = (int32_t)(511.0 * std::sin(a) + 1.0);
        cos512[i] = (int32_t)(511.0 * std::cos(a) + 1.0);
    }
    uint64_t h = 0xcbf29ce484222325ull;
    auto eat = [&h](const int32_t *t) {
        for (int i = 0; i < 512; i++)
            for (int k = 0; k < 4; k++) {
                h ^= (uint8_t)((uint32_t)t[i] >> (8 * k));
                h *= 0x100000001b3ull;
            }
    };
    eat(sin512);
    eat(cos512);
    return h == kSinCosFnv1a;
}

/* C/A code of one PRN (the table codegen() builds, plutogpssim.c:207-244), generated the ICD way:
 * two 10-stage LFSRs, G1 = 1+x^3+x^10, G2 = 1+x^2+x^3+x^6+x^8+x^9+x^10, both preset to all ones, and
 * the PRN picked by XOR-ing two G2 stages (the "phase selector"), which is equivalent to the G2 delay
 * table the reference uses (c:208-213). */
const uint8_t kG2Taps[32][2] = {
    {2, 6}, {3, 7}, {4, 8}, {5, 9}, {1, 9}, {2, 10}, {1, 8}, {2, 9}, {3, 10}, {2, 3}, {3, 4},
    {5, 6}, {6, 7}, {7, 8}, {8, 9}, {9, 10}, {1, 4}, {2, 5}, {3, 6}, {4, 7}, {5, 8}, {6, 9},
    {1, 3}, {4, 6}, {5, 7}, {6, 8}, {7, 9}, {8, 10}, {1, 6}, {2, 7}, {3, 8}, {4, 9}};

void make_ca(int prn, uint8_t ca[GPSBB_CA_LEN])
{
    /* bit k-1 of g = stage k */
    uint32_t g1 = 0x3ff, g2 = 0x3ff;
    const int t1 = kG2Taps[prn - 1][0], t2 = kG2Taps[prn - 1][1];
    for (int i = 0; i < GPSBB_CA_LEN; i++) {
        const uint32_t o1 = (g1 >> 9) & 1u;
        const uint32_t o2 = ((g2 >> (t1 - 1)) ^ (g2 >> (t2 - 1))) & 1u;
        ca[i] = (uint8_t)(o1 ^ o2);
        const uint32_t f1 = ((g1 >> 2) ^ (g1 >> 9)) & 1u;
        const uint32_t f2 = ((g2 >> 1) ^ (g2 >> 2) ^ (g2 >> 5) ^ (g2 >> 7) ^ (g2 >> 8) ^ (g2 >> 9)) & 1u;
        g1 = ((g1 << 1) | f1) & 0x3ff;
        g2 = ((g2 << 1) | f2) & 0x3ff;
    }
}

/* descriptor contract of gpsbb_chan_t (include/gpsbb.h) */
bool chan_ok(const gpsbb_chan_t &c, double delt, bool fixed = false)
{
    if (c.prn == 0)
        return true;
    if (c.prn < 0 || c.prn > 32)
        return false;
    if (!std::isfinite(c.f_carr) || !std::isfinite(c.f_code) || !std::isfinite(c.carr_phase) ||
        !std::isfinite(c.code_phase) || !std::isfinite(c.gain))
        return false;
    if (!fixed && (std::signbit(c.carr_phase) || c.carr_phase > 1.0))
        return false;
    if (fixed && (std::signbit(c.carr_phase) || c.carr_phase >= 4294967296.0 || c.carr_phase != std::floor(c.carr_phase)))
        return false; /* fixed-point variant: the value of the 32-bit accumulator */
    if (std::signbit(c.code_phase) || !(c.code_phase < 1023.0))
        return false;
    const double sc = c.f_code * delt, sk = c.f_carr * delt;
    if (!(sc > 0.0 && sc <= 1.5) || !(std::fabs(sk) <= 0.125))
        return false;
    if (!(std::fabs(c.gain) < 2097152.0))
        return false;
    if (c.iword < 0 || c.iword > 59 || c.ibit < 0 || c.ibit > 29 || c.icode < 0 || c.icode > 19)
        return false;
    for (int k = 0; k < GPSBB_N_DWRD; k++)
        if (c.dwrd[k] >> 30)
            return false;
    return true;
}

/* Upper bound on the rows build_rows() emits for one chain (see the derivation in DESIGN.md):
 * every lap (wrap to wrap) visits at most (top_e - e_s + 2) binades, each costing at most two rows,
 * plus a handful of explicit steps around the wrap. */
uint64_t row_bound(double s_abs, double range, int top_e, int nsamp)
{
    if (!(s_abs > 0.0))
        return 4;
    int es;
    std::frexp(s_abs, &es); /* s_abs = m * 2^es, m in [0.5,1)  ->  binade exponent es-1 */
    es -= 1;
    const double laps = std::floor((double)nsamp * s_abs / range) + 2.0;
    int binades = top_e - es + 3;
    if (binades < 3)
        binades = 3;
    const double per_lap = 2.0 * binades + 6.0;
    return (uint64_t)(laps * per_lap) + 16;
}

/*
 * Where a carrier will be n steps on, to ~1e-14 cycles, WITHOUT walking it: the phase pass B of the device-side chain
 * starts a segment from.  The reference's recurrence x = fl(x + s) does not advance by s per step but,
 * while x is in binade e, by s rounded to a multiple of that binade's last place (gpsbb_nco.h): a drift of
 * delta_e = RN(s / ulp_e) * ulp_e - s per step, i.e. of delta_e / |s| per unit of phase travelled there.  R(x) is that
 * density integrated from 0 to x (piecewise linear, one piece per binade from s's own up to [0.5, 1)); a path of
 * n steps from x0 covers whole laps R(1) each plus the two ends.  What is left out — the roundings of the steps that
 * cross a binade edge or wrap, and that a binade holds a whole number of steps — averages out: 6e-15 rms per 625 000
 * samples at 25 MS/s against 1e-11 for x0 + n*s (measured against the exact jump-ahead).  The chain's exactness does
 * not rest on this: fix_block takes any start phase within pass B's margin of the truth; a poor prediction only costs a
 * walk of the segment.
 */
struct CarrDrift {
    int e_lo = 0, n = 0;
    double sa = 0.0, R1 = 0.0;
    bool neg = false;
    double dens[64], cum[65];
    explicit CarrDrift(double s)
    {
        sa = std::fabs(s);
        neg = s < 0.0;
        if (!(sa >= 0x1p-60) || !(sa < 0.25))
            return; /* no model: plain arithmetic */
        int es;
        std::frexp(sa, &es);
        es -= 1; /* sa in [2^es, 2^(es+1)) */
        e_lo = es - 1 < -1 ? es - 1 : -1;
        cum[0] = 0.0;
        for (int e = e_lo; e <= -1; e++) {
            const double ulp = std::ldexp(1.0, e - 52);
            const double q = s / ulp; /* exact: a power of two */
            const double delta = (std::nearbyint(q) - q) * ulp;
            dens[n] = delta / sa;
            cum[n + 1] = cum[n] + dens[n] * std::ldexp(1.0, e); /* the binade is 2^e wide */
            n++;
        }
        R1 = cum[n];
    }
    double R(double x) const
    {
        if (n == 0 || !(x > std::ldexp(1.0, e_lo)))
            return 0.0;
        if (x >= 1.0)
            return R1;
        const int e = std::ilogb(x);
        const int k = e - e_lo;
        return cum[k] + dens[k] * (x - std::ldexp(1.0, e));
    }
    /* the phase n steps after x0 (both in [0, 1)) */
    double advance(double x0, int nsteps, double s) const
    {
        const double u = x0 + (double)nsteps * s;
        const double fl = std::floor(u), end = u - fl;
        const double drift = neg ? -fl * R1 + R(x0) - R(end) : fl * R1 + R(end) - R(x0);
        double v = end + drift;
        v -= std::floor(v);
        return v;
    }
};

/* A channel's bias W as a whole number of units of 2^-32 (rounded up): the guard format then carries exactly W — 2^20 + W is
 * representable — and not W rounded to the format's grid, half a unit of error that 1 / step would amplify. */
double ev_bias_on_grid(double w)
{
#ifdef GPSBB_W_OFF_GRID /* (measurement: rounds 2 and 3) */
    return w;
#else
    return w < 0.25 ? std::ceil(w * 4294967296.0) * 0x1p-32 : w;
#endif
}

/*
 * Can the breakpoint kernel render these blocks, and with which per-channel constants (EvConst)?  Eligible
 * when, for every active channel, a run of SPT samples holds at most one chip change (sc*15.5 < 1) and at
 * most EV_KC_MAX table-index changes, and, per block, the I sums cannot reach 2^15 (sum of 512*|gain|+1: the
 * packed I/Q arithmetic of that kernel needs it; the reference's (short) wrap-around is then unreachable
 * too).  Steps are the individually rounded products the kernels and the reference use (c:2709, 2741).
 */
bool ev_plan(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, std::vector<EvConst> &out, bool fixed = false)
{
    const size_t nbc = (size_t)nblocks * nch;
    out.resize(nbc);
    const double reach = (double)SPT - 0.5;
    for (int blk = 0; blk < nblocks; blk++) {
        double amp_sum = 0.0;
        for (int i = 0; i < nch; i++) {
            const gpsbb_chan_t &c = ch[(size_t)blk * nch + i];
            EvConst &K = out[(size_t)blk * nch + i];
            memset(&K, 0, sizeof K);
            if (c.prn <= 0)
                continue;
            amp_sum += 512.0 * std::fabs(c.gain) + 1.0;
            const volatile double sc = c.f_code * delt, sk = c.f_carr * delt;
            double S = sk * 512.0;
            if (fixed) {
                /* the 32-bit accumulator (c:2675, 2699): the table index is phase / 2^16 modulo 512, its step exactly
                 * step / 2^16.  Only k_synth_pd takes it (every channel evaluated per sample: checked below) */
                const volatile double scaled = 512.0 * 65536.0 * c.f_carr * delt;
                S = (double)(int)std::round(scaled) * 0x1p-16;
            }
            const double aS = std::fabs(S);
            /* more than one chip change per run: the channel is evaluated per sample (ev_dense), as long as the chip
             * table reaches past what a tile covers (which also leaves at most one code roll-over per tile) */
            const bool dense_code = !(sc * reach < 1.0);
            if (!(sc >= 0x1p-20) || !(1023.0 + 1040.0 * sc + 2.0 <= (double)EV_CHIP_LEN))
                return false;
            K.S = aS; /* a falling carrier is walked mirrored: phase -y, step |S| */
            K.sc = sc;
            K.rsc = 1.0 / sc;
            K.down = S < 0.0;
            /* how far an estimated change position may be off (in samples): the model's error over the step, plus the
             * roundings of the guard format (one unit in the last place is 2^-32 there) */
            const double wC = EV_MODEL_ERR * K.rsc + EV_T_EPS;
            double wK = 0.0;
            if (aS == 0.0) {
                K.rS = 0x1p+1000; /* the index never changes */
                K.kc = 1;
            } else if (aS < 8.0 * EV_MODEL_ERR) {
                K.rS = 0x1p+1000; /* the model error exceeds an eighth of a step (W would pass 1/8 sample): every run is recomputed exactly */
                K.kc = -1;
            } else {
                K.rS = 1.0 / aS;
                wK = EV_MODEL_ERR * K.rS + EV_T_EPS;
                const double kc = std::floor((reach + wK) * aS) + 1.0;
                K.kc = kc > (double)EV_KC_MAX ? EV_KC_DENSE : (int)kc; /* too many index changes per run: per sample */
            }
            /* one bias W for everything tested in the channel (first-sample fractions: W >= the model error in index units /
             * chips; change positions: W >= wK, wC): the tests are then all "low word of the biased quantity < 2W" */
            K.W = std::max(std::max(wK, wC), EV_T_EPS);
            K.W = ev_bias_on_grid(K.W);
            K.danger = K.W >= 0.25 ? 0x80000000u : (uint32_t)std::ceil(2.0 * K.W * 4294967296.0) + 1u;
            {
                /* (test aid, experiments build: a larger threshold sends more lane-runs to the exact path; never a smaller one) */
                const long floor_ = GPSBB_KNOB_LONG("GPSBB_EV_DANGER", 0);
                if (floor_ > 0 && (uint32_t)floor_ > K.danger)
                    K.danger = (uint32_t)floor_;
            }
            K.tK0 = K.rS * (1.0 + K.W) + 0x1p+20 + K.W;
            K.tC0 = K.rsc * (1.0 + K.W) + 0x1p+20 + K.W;
            K.pd_S8 = aS * 8.0;
            K.pd_dy = aS * 512.0;
            K.pd_sc2 = sc * 2.0;
            K.pd_dx = sc * 128.0;
            if (dense_code && K.kc > 0)
                K.kc = EV_KC_DENSE;
            if (fixed) {
                /* The accumulator's index model is exact (gpsbb_events.hip.h, ev_first<KC, true>): nothing on the carrier side is
                 * biased or tested, the change positions come from (1 - fraction - 2^-17) / |step|.  Per sample (k_synth_pd) where
                 * a run holds more than one chip change, per breakpoint otherwise; what neither takes goes to the stepped kernel. */
                if (dense_code) {
                    if (!(aS < 64.0))
                        return false;
                    K.kc = EV_KC_DENSE;
                } else {
                    const double kc = std::floor(reach * aS) + 1.0;
                    if (kc > (double)EV_KC_MAX)
                        return false;
                    K.kc = (int)kc;
                    K.rS = aS > 0.0 ? 1.0 / aS : 0x1p+1000;
                    K.W = ev_bias_on_grid(std::max(wC, EV_T_EPS));
                    K.danger = K.W >= 0.25 ? 0x80000000u : (uint32_t)std::ceil(2.0 * K.W * 4294967296.0) + 1u;
                    K.tK0 = K.rS * (1.0 - 0x1p-17) + 0x1p+20;
                    K.tC0 = K.rsc * (1.0 + K.W) + 0x1p+20 + K.W;
                }
            }
            /* what k_synth_ev's channel loop would otherwise work out per channel and tile in scalar instructions */
            K.danger_le = K.kc < 0 ? 0xffffffffu : K.danger - 1u; /* danger >= 1 */
            K.chip_at = (uint32_t)(offsetof(EvLdsLean, chip2) + (size_t)i * sizeof(uint16_t) * EvLdsLean::CHIPS) - (EV_GUARD_HI << 1);
            K.amp_at = (uint32_t)(offsetof(EvLdsLean, amp) + (size_t)i * sizeof(uint32_t) * EvLdsLean::AMP) - (EV_GUARD_HI << 2);
        }
        if (!(amp_sum < 32768.0))
            return false;
    }
    return true;
}

/* Does the lap-parallel pre-pass take these blocks (gpsbb_laps.hip.h, Eligibility)?  It is exact for any step it walks; what is
 * excluded is what its turn of the walk does not cover: steps more than 50 binades below the state (0 < |step| < 2^-50: below
 * 2e-8 Hz at 25 MS/s).  A step of exactly zero — a carrier without Doppler — is taken: the phase stands still (round 6). */
bool lap_carr_step_ok(double f_carr, double delt) /* the carrier's condition alone (gpsbb_chain_carrier has no code chains) */
{
    const volatile double sk = f_carr * delt;
    return std::fabs(sk) >= 0x1p-50 || sk == 0.0; /* (exactly zero stands still: lap_run takes it) */
}

bool lap_eligible(const gpsbb_chan_t *ch, size_t nbc, double delt, bool fixed)
{
    for (size_t k = 0; k < nbc; k++) {
        const gpsbb_chan_t &c = ch[k];
        if (c.prn <= 0)
            continue;
        const volatile double sc = c.f_code * delt;
        if (!(sc >= 0x1p-20))
            return false;
        if (!fixed && !lap_carr_step_ok(c.f_carr, delt))
            return false;
    }
    return true;
}

/* room for the laps of every channel, in chunks of LAP_WG lanes: a chain of n steps of size s wraps at most floor(n * s / range)
 * + 1 times, a block may start a chain (one more lap), and the model's step differs from s by parts in 10^12 */
/* laps a lane walks (LapDev::unit): what a lane costs besides its walk is about one lap's walk (measured: 17 turns of ~55
 * vector instructions against ~900 for finding the lap, the model, the scan and the record), so a lane takes a few */
/* (GPSBB_LAP_UNIT_CODE = 0: a block's whole code chain in one lane — it starts from a known state, so nothing but the walk itself
 * is needed: 14 % fewer instructions, and measured SLOWER, 5.22e11 against 5.39e11: what a neighbour costs the synthesis kernel
 * is the time its wavefronts sit on a SIMD, not what they issue; a hundred laps in a row sit 0.4 ms) */
constexpr int LAP_UNIT_CARR = 4, LAP_UNIT_CODE = 2;
/* a burst of plain steps (lap_run) for the lanes that are due one when they are at least 1 / LAP_BURST_SHARE of the lanes still walking */
constexpr int LAP_BURST_SHARE = 4;
/* ... where there are lanes to spare: a batch of a few block-channels (one block: the drop-in call, whose LATENCY is the point)
 * has a few thousand laps for 1024 SIMDs — a lane per lap there (gpsbb_fill_block of the reference's geometry: 0.25 against
 * 0.31 ms) */
int lap_unit(int kind, size_t nbc)
{
    long u = kind == NCO_CARR ? GPSBB_KNOB_LONG("GPSBB_LAP_UNIT_CARR", LAP_UNIT_CARR) : GPSBB_KNOB_LONG("GPSBB_LAP_UNIT_CODE", LAP_UNIT_CODE);
    if (nbc <= 256)
        u = 1;
    else if (nbc <= 1024)
        u = kind == NCO_CARR ? std::min(u, 2L) : 1L;
    if (kind == NCO_CODE && u == 0)
        return 0; /* one lane per block: a code chain is a block long and starts from its descriptor's code_phase (c:2673) */
    return u < 1 ? 1 : (u > 64 ? 64 : (int)u);
}

void lap_bound(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp, bool fixed, uint32_t chunk0[2][GPSBB_MAX_CHAN + 1],
               bool carr_only = false)
{
    for (int kind = 0; kind < 2; kind++) {
        chunk0[kind][0] = kind == 0 ? 0u : chunk0[0][GPSBB_MAX_CHAN]; /* one array of chunks: the code chains', then the carriers' */
        for (int i = 0; i < nch; i++) {
            double laps = 0.0;
            for (int blk = 0; blk < nblocks; blk++) {
                const gpsbb_chan_t &c = ch[(size_t)blk * nch + i];
                if (c.prn <= 0 || (kind == NCO_CARR && fixed) || (kind == NCO_CODE && carr_only))
                    continue;
                const double s = kind == NCO_CARR ? std::fabs(c.f_carr * delt) : c.f_code * delt * (1.0 / 1023.0);
                /* (wraps, in lanes of `unit` laps, + a head and the rounding) */
                laps += std::floor((std::floor((double)nsamp * s * (1.0 + 0x1p-30)) + 1.0) / (double)std::max(1, lap_unit(kind, (size_t)nblocks * nch))) + 3.0;
            }
            const uint32_t chunks = (uint32_t)((laps + (double)(LAP_WG - 1)) / (double)LAP_WG) + 1u;
            chunk0[kind][i + 1] = chunk0[kind][i] + chunks;
        }
        for (int i = nch; i < GPSBB_MAX_CHAN; i++)
            chunk0[kind][i + 1] = chunk0[kind][i];
    }
}

} /* namespace */

/* ================================================================================================== */
/* handle / batch                                                                                     */
/* ================================================================================================== */

/* A few host threads that stay around between calls (host-side seeding of small batches): starting two
 * dozen threads costs more than the work they are given. */
struct WorkPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    std::function<void(size_t)> job;
    size_t njobs = 0, next = 0, running = 0;
    unsigned long gen = 0;
    bool stop = false;

    explicit WorkPool(size_t nworkers)
    {
        for (size_t t = 0; t < nworkers; t++)
            th.emplace_back([this] { loop(); });
    }
    ~WorkPool()
    {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cv_work.notify_all();
        for (auto &t : th)
            t.join();
    }
    void loop()
    {
        unsigned long seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv_work.wait(lk, [&] { return stop || gen != seen; });
            if (stop)
                return;
            seen = gen;
            drain(lk);
        }
    }
    /* take jobs until none is left; called with the lock held */
    void drain(std::unique_lock<std::mutex> &lk)
    {
        running++;
        while (next < njobs) {
            const size_t j = next++;
            lk.unlock();
            job(j);
            lk.lock();
        }
        if (--running == 0)
            cv_done.notify_all();
    }
    /* run f(0..n-1) on the workers and the calling thread; returns when all are done */
    void run(size_t n, std::function<void(size_t)> f)
    {
        std::unique_lock<std::mutex> lk(m);
        job = std::move(f);
        njobs = n;
        next = 0;
        gen++;
        cv_work.notify_all();
        drain(lk);
        cv_done.wait(lk, [&] { return running == 0 && next >= njobs; });
        njobs = 0;
    }
};

constexpr int SEED_STREAMS_MAX = 8;
constexpr int CHAIN_SEG_ROWS = 1750;    /* rows of a carrier chain per segment of the device-side chain, about (see plan_segments) */
constexpr int CHAIN_SEG_MIN_TILES = 16; /* ... but no segment shorter than this many tiles */
constexpr int CHAIN_SEG_MAX = 8;        /* segments per block at most */
constexpr int CHAIN_INDEP_MIN_TILES = 1024; /* independent blocks of at least this many tiles are cut into segments as well */
constexpr long CHAIN_MODEL_MAX_SEGS = 4096; /* segments per channel up to which pass B starts from the host's drift model */
constexpr unsigned STREAM_SEED_STREAMS = 2; /* pre-passes of a stream's pushes in flight.  Round 6, the lap-parallel pre-pass beside a synthesis
                                               kernel that keeps every CU to the end of its launch: for ONE handle 2, 3 and 4 give the same rate
                                               (5.43 - 5.60e11 at 12 hardware queues, tools/sweep_seed_streams.sh: what is in flight shares the
                                               slots the synthesis leaves).  Two it is: with the synthesis stream and the process's null stream
                                               that makes the four hardware queues HIP maps streams onto by default, so every one of them has a
                                               queue to itself: a pre-pass that shares a queue with the synthesis, or with a stream that holds a
                                               wait for one, runs after it and not beside it */

/* How many of each kind of resource this process holds right now (gpsbb_test_live): counted where an owner's allocation succeeds
 * and where it releases.  A launch never allocates, so none of this is on a hot path. */
static std::atomic<long long> g_live_dev{0}, g_live_pinned{0}, g_live_events{0};
static void live_add(std::atomic<long long> &n, long long d) { n.fetch_add(d, std::memory_order_relaxed); }

/* device memory that is kept between calls and only ever grows */
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0; /* elements */
    /* room: a first allocation that expects to be outgrown (the row pool of a ring slot, whose pushes see different
     * Dopplers) takes that much more than asked, so that the stream does not stall on re-allocations later */
    int reserve(size_t n, size_t room = 0)
    {
        if (n <= cap)
            return hipSuccess;
        n += room;
        if (p)
            n += n / 4; /* the free synchronises the device: grow with head-room so that a ring whose slots see
                           slightly different row counts stops re-allocating after a few pushes */
        release();
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = n;
        live_add(g_live_dev, 1);
        return hipSuccess;
    }
    void release()
    {
        if (p) {
            (void)hipFree(p);
            live_add(g_live_dev, -1);
        }
        p = nullptr;
        cap = 0;
    }
};

/* pinned host memory, likewise: what is outgrown comes back as n + room elements, and each site says how much room it wants */
template <class T>
struct PinnedBuf {
    T *p = nullptr;
    size_t cap = 0; /* elements */
    int reserve(size_t n, size_t room = 0)
    {
        if (n <= cap)
            return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void **)&p, (n + room) * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = n + room;
        live_add(g_live_pinned, 1);
        return hipSuccess;
    }
    void release()
    {
        if (p) {
            (void)hipHostFree(p);
            live_add(g_live_pinned, -1);
        }
        p = nullptr;
        cap = 0;
    }
};

/* an event, made once: hipEventDefault for the ones whose times are read, hipEventDisableTiming for the ones that only order */
struct Event {
    hipEvent_t e = nullptr;
    hipError_t make(unsigned flags)
    {
        if (e)
            return hipSuccess;
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc != hipSuccess)
            e = nullptr;
        else
            live_add(g_live_events, 1);
        return rc;
    }
    void release()
    {
        if (e) {
            (void)hipEventDestroy(e);
            live_add(g_live_events, -1);
        }
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

/* release() of every owner named (DevBuf, PinnedBuf, Event, or a struct of them) */
template <class... B>
static void release_all(B &...b)
{
    (b.release(), ...);
}

/* ... of a call's own temporaries, on every way out of it: const AtExit done{[&] { release_all(a, b); }}; */
template <class F>
struct AtExit { F f; ~AtExit() { f(); } };
template <class F> AtExit(F) -> AtExit<F>;

/* Two events around the kernels of a call's last run, for the experiments build's gpsbb_test_*_ms hooks: without
 * GPSBB_EXPERIMENTS start and stop do nothing, and no event is ever made. */
struct KernelTimer {
    Event ev[2];
    hipError_t start(hipStream_t stream)
    {
#ifdef GPSBB_EXPERIMENTS
        for (Event &e : ev) {
            const hipError_t rc = e.make(hipEventDefault);
            if (rc != hipSuccess)
                return rc;
        }
        return hipEventRecord(ev[0], stream);
#else
        return hipSuccess;
#endif
    }
    hipError_t stop(hipStream_t stream)
    {
#ifdef GPSBB_EXPERIMENTS
        return hipEventRecord(ev[1], stream);
#else
        return hipSuccess;
#endif
    }
    /* milliseconds between the two, once both have happened; -1: nothing was timed yet */
    float ms() const
    {
        float t = -1.0f;
        return ev[0] && ev[1] && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess ? t : -1.0f;
    }
    void release() { release_all(ev[0], ev[1]); }
};

struct gpsbb {
    int device = 0;
    /* The streams.  gpsbb_create makes the first three: with the process's null stream they are what the steady state
     * of a chained ring or of a re-run batch keeps busy, one hardware queue each at HIP's default of four.  The others exist once
     * something has asked for them. */
    hipStream_t s_seed = nullptr;    /* pre-pass: the descriptor and plan uploads of a set-up, then the NCO pre-pass (k_lap_*, k_seed, ...) */
    hipStream_t s_more[SEED_STREAMS_MAX - 1] = {}; /* ... [0] the second one: every other batch, every other push of a stream, every other
                                                      run of a batch with three table sets (batch_prepass_stream); [1..] experiments only */
    unsigned batches_created = 0;
    hipStream_t s_compute = nullptr; /* synthesis kernel, and what merely follows it in order: a device-only ring's end states and digests */
    hipStream_t s_compute2 = nullptr; /* (experiments, GPSBB_TWO_COMPUTE_STREAMS: the synthesis of every other launch; created on first use) */
    unsigned compute_turn = 0;
    hipStream_t s_copy = nullptr;    /* host-bound output of a ring: gather, pack and noise kernels into pinned memory; created by the first
                                        push that has any.  A device-only ring never touches it */
    hipStream_t s_digest = nullptr;  /* gpsbb_slot_digest, created on first use: a stream nothing else waits on (the copy stream holds a
                                        wait for every push in flight: a digest queued there ran when the whole ring had drained) */
    std::vector<uint32_t> h_ca;      /* host copy of the C/A chips (seeding of small batches on the host)  */
    unsigned long long host_dwrd_oob = 0, host_itable_512 = 0; /* hazards counted by host-side seeding      */
    WorkPool *pool = nullptr;        /* host threads for seeding small batches (created on first use)      */
    DevBuf<int32_t> d_tabs;
    DevBuf<uint32_t> d_ca;
    DevBuf<uint32_t> d_status;
    DevBuf<unsigned long long> d_hz;
    DevBuf<unsigned long long> d_clip;  /* GPSBB_INFO_SC8_CLIPPED: the packing kernels add their saturated components here */
    DevBuf<int2> d_noise_tab;           /* the noise's knots (K[i], K[i + 1] - K[i]) and ... */
    DevBuf<unsigned long long> d_nclip; /* ... GPSBB_INFO_NOISE_CLIPPED: both on the first call with noise, both or neither */
    int last_hip = 0;
    gpsbb_batch *scratch = nullptr;
    PinnedBuf<unsigned char> h_bounce; /* a fill whose iq_out lies partly in a registered range is copied through here */
    PinnedBuf<unsigned char> h_fill;   /* what the drop-in call brings back besides the IQ — the end states and the status word
                                          (fill_block_finish) */
    struct HostReg { char *host; char *dev; size_t bytes; };
    std::vector<HostReg> host_regs;         /* gpsbb_host_register: host ranges the device writes straight into */
    struct ChainOnly *chain_only = nullptr; /* device scratch of gpsbb_chain_carrier, kept between calls */
    int sm_count = 0;
    /* per-handle options (gpsbb_set_option) */
    int opt_seed_where = 0;   /* 0 by size (on the device: lap-parallel where eligible), 1 always the row walks (k_seed / k_walk), 2 always
                                 host threads, 3 always on the device, lap-parallel where eligible */
    int opt_synth_kernel = 0; /* 0 automatic, 1 always the per-sample kernel */
    int opt_skip_seed = 0;    /* measurement: re-use the tables of the first two runs of a batch */
    int opt_chain_where = 0;  /* GPSBB_CHAIN_CARRIER: 0 automatic (on the device wherever the pre-pass runs there), 1 host threads,
                                 2 as 0 with the fix-up walking the blocks in order (k_chain_fix instead of k_chain_fix_par) */
    int last_kernel = 0;      /* synthesis kernel of the last launch: 1 per-sample, 2 breakpoint */
    int last_variant = 0;     /* ... and which one exactly: GPSBB_VARIANT_* */
    int last_chain_dev = 0;   /* the last launch resolved GPSBB_CHAIN_CARRIER on the device */
    int last_prepass = 0;     /* pre-pass of the last launch: 1 row walks on the device, 2 host threads, 3 lap-parallel on the device */
    /* The scratch of the calls that read device IQ, null until the first call that needs it and kept between calls.  One that is
     * outgrown comes back a quarter larger than asked (DevBuf::reserve): more memory held, the same results. */
    DevBuf<unsigned char> d_pack;          /* a packed fill's / gpsbb_device_pack's bytes */
    DevBuf<LevelOut> d_level;              /* gpsbb_device_level's result, per block */
    DevBuf<unsigned long long> d_digest;   /* gpsbb_device_digest's and gpsbb_slot_digest's sums, per block */
    DevBuf<unsigned long long> d_acq_chips, d_acq_rows; /* gpsbb_device_acquire's (in 8-byte words): the expanded chips; the tiles'
                                                           partials with the rows behind them */
    DevBuf<unsigned long long> d_acq_grid; /* ... and the grid where wanted (up to 512 MiB, for tests and plots): released when the call
                                              that asked for it has copied it out, here only while that call runs or after it failed:
                                              but for that, a first allocation every time, of exactly what was asked */
    DevBuf<unsigned long long> d_trk;      /* gpsbb_device_track's: the states, the counts, the records */
    DevBuf<unsigned long long> d_fir;      /* gpsbb_device_fir's: the clip count, the two histories */
    DevBuf<unsigned long long> d_psd_tab;  /* gpsbb_device_psd's: the twiddles as k_psd reads them (uploaded once), the window, the result */
    DevBuf<unsigned long long> d_psd;      /* ... and the workgroups' partials */
    DevBuf<unsigned long long> d_exc;      /* gpsbb_device_excise's: the inverse's tables (uploaded once), the plan, the histories, the counts */
    DevBuf<unsigned long long> d_blank;    /* gpsbb_device_blank's: the histories, the counts */
    KernelTimer acq_tm, trk_tm, fir_tm, psd_tm, exc_tm, blank_tm; /* around the kernels of the last gpsbb_device_acquire, _track, _fir, _psd, _excise, _blank (gpsbb_test_*_ms) */
};

/* every stream the handle has created, in no particular order */
template <class F>
static void for_each_stream(const gpsbb *h, F f)
{
    for (hipStream_t st : {h->s_seed, h->s_compute, h->s_compute2, h->s_copy, h->s_digest})
        if (st)
            f(st);
    for (hipStream_t st : h->s_more)
        if (st)
            f(st);
}

/* Wait for everything the handle has enqueued, whichever stream holds it: before memory any of it may touch is freed,
 * unregistered or read by the host (gpsbb_sync, the destroy calls, gpsbb_host_unregister).  An idle stream costs a call. */
static hipError_t drain_streams(const gpsbb *h)
{
    hipError_t first = hipSuccess;
    for_each_stream(h, [&](hipStream_t st) {
        const hipError_t e = hipStreamSynchronize(st);
        if (first == hipSuccess)
            first = e;
    });
    return first;
}

/* The lap-parallel pre-pass's device scratch (gpsbb_laps.hip.h: what LapDev points at): one per table set of a batch, one for
 * gpsbb_chain_carrier. */
struct LapScratch {
    DevBuf<LapBC> bc;
    DevBuf<uint32_t> lane0, cnt, chunk_bad;
    DevBuf<LapRec> rec;
    DevBuf<LapAgg> agg;
    DevBuf<double> chunk_m;
    /* room for `chunks` chunks of laps over nbc = nblocks * nch block-channels; `room`: a quarter more of what grows with the laps
     * on a first allocation (a ring slot, whose pushes see different Dopplers: DevBuf::reserve) */
    int reserve(size_t nbc, size_t nch, size_t nblocks, size_t chunks, bool room)
    {
        const size_t more = room ? chunks / 4 : 0;
        int e = bc.reserve(2 * nbc); /* (each step only if the ones before it succeeded: hipSuccess is 0) */
        e = e ? e : lane0.reserve(2 * nch * (nblocks + 1));
        e = e ? e : cnt.reserve(4 * GPSBB_MAX_CHAN);
        e = e ? e : rec.reserve(chunks * LAP_WG, room ? chunks * LAP_WG / 4 : 0);
        e = e ? e : agg.reserve(chunks, more);
        e = e ? e : chunk_m.reserve(chunks, more);
        return e ? e : chunk_bad.reserve(chunks, more);
    }
    void release() { release_all(bc, lane0, cnt, chunk_bad, rec, agg, chunk_m); }
    void dev(LapDev &L) const
    {
        L.bc = bc.p;
        L.lane0 = lane0.p;
        L.nlaps = cnt.p;
        L.nbad = cnt.p + 2 * GPSBB_MAX_CHAN;
        L.rec = rec.p;
        L.agg = agg.p;
        L.chunk_m = chunk_m.p;
        L.chunk_bad = chunk_bad.p;
    }
};

/* k_chain_fix_par's hand-off between its chunks (BatchDev::fix_end, fix_flag, fix_epoch): a batch has one, cut into a piece per
 * table set, gpsbb_chain_carrier another. */
struct FixScratch {
    DevBuf<unsigned long long> end;
    DevBuf<int> flag;
    bool flags_zeroed = false; /* `flag` has been cleared since it was last (re)allocated */
    int epoch = 0;             /* the last number handed to k_chain_fix_par */
    /* flags are compared with a launch number, never cleared: zeroed once, when the buffer is (re)allocated */
    hipError_t reserve(size_t nflags, hipStream_t stream)
    {
        if (nflags <= flag.cap && end.cap >= flag.cap && flags_zeroed)
            return hipSuccess;
        /* (all three steps or none: a set-up that failed half-way must not leave flags that were never zeroed, or no
         * buffer for the end phases, behind a capacity that says "nothing to do") */
        flags_zeroed = false;
        hipError_t e = (hipError_t)flag.reserve(nflags);
        e = e ? e : (hipError_t)end.reserve(flag.cap);
        e = e ? e : hipMemsetAsync(flag.p, 0, flag.cap * sizeof(int), stream);
        if (e != hipSuccess)
            return e;
        epoch = 0;
        flags_zeroed = true;
        return hipSuccess;
    }
    void release() { release_all(end, flag); }
};

/* A stream's two events (gpsbb_batch::ev_prefix, ev_fix), or none: a batch that continues no push.  They order what touches the
 * stream's carry (ChainCarryDev) across pushes, which take the handle's pre-pass streams in turn. */
struct CarryEvents {
    hipEvent_t prefix = nullptr, fix = nullptr;
    static hipError_t wait(hipStream_t ss, hipEvent_t e) { return e ? hipStreamWaitEvent(ss, e, 0) : hipSuccess; }
    static hipError_t record(hipStream_t ss, hipEvent_t e) { return e ? hipEventRecord(e, ss) : hipSuccess; }
    /* The lap-parallel pre-pass: the carry is read by a push's carrier plan and written by its repair (exact_end AND approx_end):
     * ordered behind every writer of the push before — lap-parallel or row walks — and ahead of every reader of the next, whichever
     * pre-pass that push takes: both events waited for, both recorded */
    hipError_t wait_both(hipStream_t ss) const
    {
        const hipError_t e = wait(ss, fix);
        return e ? e : wait(ss, prefix);
    }
    hipError_t record_both(hipStream_t ss) const
    {
        const hipError_t e = record(ss, fix);
        return e ? e : record(ss, prefix);
    }
};

/* What a batch owns per table set: the tables a pre-pass leaves and a synthesis kernel reads, the pre-pass's scratch, and when
 * the set is free again. */
struct TableSet {
    DevBuf<NcoRow> rows;
    DevBuf<int32_t> tile_row;
    DevBuf<int32_t> row_cnt;
    DevBuf<gpsbb_chan_state_t> end;
    /* breakpoint kernel (ev): exact tile-start states instead of rows + tile index */
    DevBuf<double> tile_x;
    DevBuf<uint32_t> tile_nav;
    /* GPSBB_CHAIN_CARRIER resolved on the device by the row walks (gpsbb_walk.hip.h) */
    DevBuf<ChainAux> aux;
    DevBuf<SynRow> prefix;
    LapScratch lap; /* the lap-parallel pre-pass (gpsbb_laps.hip.h): one lane per lap of every chain */
    hipEvent_t synth_done_ref = nullptr; /* not owned: ev[3] of the run that last read this set */
    bool synth_pending = false;
    void release() { release_all(rows, tile_row, row_cnt, end, tile_x, tile_nav, aux, prefix, lap); }
};

/* Table sets of a batch.  Run k uses set k % nsets and its pre-pass may start as soon as the synthesis kernel
 * that last read that set has finished.  Three sets, and consecutive runs seed on alternating streams: a
 * pre-pass is as long as its longest chain whatever the batch size — longer than the synthesis it feeds — so
 * two of them have to be in flight for the synthesis kernel to set the pace; four, three pre-passes in flight on
 * three streams, where the carrier is chained on the device (two walks and the fix-up per run). */
constexpr int NSETS = 6;

/* GPSBB_PUSH_TRACE=<ms>: where the host time of a stream push goes, printed for pushes that take longer than <ms> */
struct PushTrace {
    double limit_ms = -1.0;
    int n = 0;
    const char *what[32];
    std::chrono::steady_clock::time_point t[32];
    PushTrace()
    {
#ifdef GPSBB_EXPERIMENTS
        const char *e = getenv("GPSBB_PUSH_TRACE");
        if (e)
            limit_ms = atof(e);
#endif
    }
    void start() { n = 0; mark("start"); }
    void mark(const char *w)
    {
        if (limit_ms < 0.0 || n >= 32)
            return;
        what[n] = w;
        t[n++] = std::chrono::steady_clock::now();
    }
    void end()
    {
        if (limit_ms < 0.0 || n < 2)
            return;
        mark("end");
        const double tot = std::chrono::duration<double, std::milli>(t[n - 1] - t[0]).count();
        if (tot < limit_ms)
            return;
        fprintf(stderr, "[gpsbb push %.3f ms]", tot);
        for (int i = 1; i < n; i++)
            fprintf(stderr, " %s %.3f", what[i], std::chrono::duration<double, std::milli>(t[i] - t[i - 1]).count());
        fprintf(stderr, "\n");
    }
};
static thread_local PushTrace g_push_trace;
#define PUSH_MARK(w) g_push_trace.mark(w)

/* carry[i] = {prn, phase} of channel i after the previous call (in) / after this one (out); may be NULL */
struct ChainCarry {
    int prn[GPSBB_MAX_CHAN];
    double phase[GPSBB_MAX_CHAN];
};
static void chain_carrier_host(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp, double *seed,
                               int nthreads, ChainCarry *carry);

/* work(i0, i1) over the channels [0, nch) in nthreads equal shares, a thread each.  A thread that cannot be started (no exception
 * may cross the C boundary) leaves its share to the caller. */
template <class Work>
static void channel_threads(int nch, int nthreads, const Work &work)
{
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++) {
        const int i0 = (int)((long)nch * t / nthreads), i1 = (int)((long)nch * (t + 1) / nthreads);
        try {
            th.emplace_back(work, i0, i1);
        } catch (...) {
            work(i0, i1);
        }
    }
    for (auto &t : th)
        t.join();
}

#include "gpsbb_plan.h"

struct gpsbb_batch {
    gpsbb *h = nullptr;
    /* the handle's seeding stream, or (odd slots of a ring) its second one: the pre-passes of two consecutive
     * slots — a few wavefronts each, as long as one chain takes — then run side by side (16-block slots:
     * 6.6e9 -> 7.3e9 samples/s at depth 3, 8.4e9 at depth 4).  Two, not one per slot: with the compute and
     * copy streams that makes four, and streams beyond the hardware queues share them. */
    hipStream_t seed_stream = nullptr;
    bool one_stream = false;       /* the drop-in call's scratch batch: upload, pre-pass and synthesis on the synthesis stream (a
                                      hop from stream to stream is 16 us of nothing for a call that takes 150: gpsbb_fill_block_ex) */
    int max_sets = NSETS;
    BatchPlan plan;  /* written by batch_setup alone, once plan_batch has succeeded */
    PlanImages img;  /* ... with it */
    StreamLink link; /* a stream's, for the length of one push */

    /* device buffers */
    DevBuf<gpsbb_chan_t> d_ch;
    DevBuf<uint64_t> d_row_off;
    /* run k uses set k % nsets, so that the seeding pre-pass of run k+1 overlaps the synthesis kernel of run k (different streams) */
    TableSet sets[NSETS];
    DevBuf<int32_t> d_tile_ctr;
    DevBuf<int32_t> d_seed_order;
    DevBuf<uint32_t> d_kph0;
    DevBuf<int32_t> d_kstep;
    DevBuf<EvConst> d_evc;
    DevBuf<int32_t> d_chain_order;
    DevBuf<ChainDesc> d_cd;
    DevBuf<double> d_start0;
    FixScratch fix;              /* k_chain_fix_par: the hand-off between its chunks, one piece per table set */
    DevBuf<int16_t> d_iq;
    DevBuf<unsigned long long> d_dig;
    /* pinned staging arena of the uploads of one set-up: hipMemcpyAsync from pageable memory is not asynchronous
     * (it waits for the stream's earlier work — the previous push's pre-pass — before it returns) */
    PinnedBuf<char> stage;
    size_t stage_used = 0;
    Event upload_done; /* descriptors and plans of the last set-up are on the device */
    hipStream_t upload_stream = nullptr; /* ... the stream that carried them */

    /* per-launch state */
    bool want_digest = false;      /* this launch also leaves every block's digest in d_dig (GPSBB_PUSH_DIGEST): by the synthesis kernel
                                      itself where there is a variant that does (k_synth_ev_digest), by k_block_digest behind it otherwise */
    hipStream_t last_cs = nullptr; /* the synthesis stream of the last launch */
    hipEvent_t last_done = nullptr;
    unsigned run_count = 0;
    int last_set = 0;
    struct Ev4 { /* seed start/end (seed stream), synth start/end (compute stream) */
        Event e[4];
        void release() { release_all(e[0], e[1], e[2], e[3]); }
    };
    std::vector<Ev4> evs; /* one set per run since the last timing reset */
    size_t ev_used = 0;
    bool ran = false;
    int16_t *last_iq = nullptr;
    int16_t *last_ext_iq = nullptr; /* the caller's device buffer of the last run, if it used one */

    /* seeding on the host (small batches): pinned images of the row pool, tile index and end states, or (ev) of the tile states */
    PinnedBuf<SynRow> hs_rows;
    PinnedBuf<int32_t> hs_tile_row;
    PinnedBuf<gpsbb_chan_state_t> hs_end;
    PinnedBuf<double> hs_tile_x;
    PinnedBuf<uint32_t> hs_tile_nav;

    /* gpsbb_batch_despread's scratch, kept between calls: the sums (and behind them the count of samples that took the exact
     * path), the tile counters */
    DevBuf<unsigned long long> d_ds;
    DevBuf<int32_t> d_ds_ctr;
    unsigned long long ds_last_exact = 0;
    KernelTimer ds_tm; /* around the last k_despread (gpsbb_test_despread_ms) */
};

#define HIPCHK(h, call)                                                                            \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            (h)->last_hip = (int)e__;                                                              \
            return e__ == hipErrorOutOfMemory ? GPSBB_E_NOMEM : GPSBB_E_HIP;                       \
        }                                                                                          \
    } while (0)

extern "C" int gpsbb_version(void) { return GPSBB_VERSION; }

extern "C" const char *gpsbb_strerror(int err)
{
    switch (err) {
    case GPSBB_OK: return "ok";
    case GPSBB_E_BADARG: return "bad argument";
    case GPSBB_E_BADCHAN: return "channel descriptor outside the contract";
    case GPSBB_E_HIP: return "HIP runtime error";
    case GPSBB_E_NOMEM: return "out of memory";
    case GPSBB_E_INTERNAL: return "device self-check failed (row pool overflow)";
    case GPSBB_E_NODEVICE: return "no usable HIP device";
    case GPSBB_E_STATE: return "call sequence violation";
    default: return "unknown error";
    }
}

extern "C" int gpsbb_last_hip_error(const gpsbb_t *h) { return h ? h->last_hip : 0; }

extern "C" int gpsbb_set_option(gpsbb_t *h, int option, long value)
{
    if (!h)
        return GPSBB_E_BADARG;
    switch (option) {
    case GPSBB_OPT_SEED_WHERE:
        if (value < 0 || value > 3)
            return GPSBB_E_BADARG;
        h->opt_seed_where = (int)value;
        return GPSBB_OK;
    case GPSBB_OPT_SYNTH_KERNEL:
        if (value < 0 || value > 1)
            return GPSBB_E_BADARG;
        h->opt_synth_kernel = (int)value;
        return GPSBB_OK;
    case GPSBB_OPT_SKIP_SEED:
        h->opt_skip_seed = value != 0;
        return GPSBB_OK;
    case GPSBB_OPT_CHAIN_WHERE:
        if (value < 0 || value > 3)
            return GPSBB_E_BADARG;
        h->opt_chain_where = (int)value;
        return GPSBB_OK;
    default:
        return GPSBB_E_BADARG;
    }
}

extern "C" int gpsbb_get_info(gpsbb_t *h, int what, uint64_t *out)
{
    if (!h || !out)
        return GPSBB_E_BADARG;
    switch (what) {
    case GPSBB_INFO_LAST_KERNEL:
        *out = (uint64_t)h->last_kernel;
        return GPSBB_OK;
    case GPSBB_INFO_LAST_VARIANT:
        *out = (uint64_t)h->last_variant;
        return GPSBB_OK;
    case GPSBB_INFO_EXACT_RUNS:
    case GPSBB_INFO_CHAIN_FALLBACKS:
    case GPSBB_INFO_CHAIN_TIES:
    case GPSBB_INFO_CHAIN_REPAIRS:
    case GPSBB_INFO_TILES_RENDERED: {
        HIPCHK(h, hipSetDevice(h->device));
        unsigned long long v = 0;
        HIPCHK(h, hipMemcpy(&v, h->d_hz.p + (what == GPSBB_INFO_EXACT_RUNS ? 2 : (what == GPSBB_INFO_CHAIN_FALLBACKS ? 4 : (what == GPSBB_INFO_CHAIN_TIES ? 5 : (what == GPSBB_INFO_TILES_RENDERED ? 7 : 6)))), 8,
                            hipMemcpyDeviceToHost));
        *out = v;
        return GPSBB_OK;
    }
    case GPSBB_INFO_SC8_CLIPPED: {
        HIPCHK(h, hipSetDevice(h->device));
        unsigned long long v = 0;
        HIPCHK(h, hipMemcpy(&v, h->d_clip.p, 8, hipMemcpyDeviceToHost));
        *out = v;
        return GPSBB_OK;
    }
    case GPSBB_INFO_NOISE_CLIPPED: {
        unsigned long long v = 0;
        if (h->d_nclip.p) {
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipMemcpy(&v, h->d_nclip.p, 8, hipMemcpyDeviceToHost));
        }
        *out = v;
        return GPSBB_OK;
    }
    case GPSBB_INFO_CHAIN_ON_DEVICE:
        *out = (uint64_t)h->last_chain_dev;
        return GPSBB_OK;
    case GPSBB_INFO_PREPASS:
        *out = (uint64_t)h->last_prepass;
        return GPSBB_OK;
    case GPSBB_INFO_STREAMS: {
        uint64_t n = 1; /* the process's null stream: the library's blocking copies run there, and it holds a hardware queue */
        for_each_stream(h, [&](hipStream_t) { n++; });
        *out = n;
        return GPSBB_OK;
    }
    case GPSBB_INFO_HW_QUEUES: {
        /* reported, never acted on: what the runtime was (or will be) told when it maps streams onto hardware queues */
        const char *e = getenv("GPU_MAX_HW_QUEUES");
        const long v = e ? atol(e) : 4;
        *out = (uint64_t)(v > 0 ? v : 4);
        return GPSBB_OK;
    }
    default:
        return GPSBB_E_BADARG;
    }
}

extern "C" int gpsbb_codegen(int prn, uint8_t ca[GPSBB_CA_LEN])
{
    if (!ca || prn < 1 || prn > 32)
        return GPSBB_E_BADARG;
    make_ca(prn, ca);
    return GPSBB_OK;
}

extern "C" int gpsbb_sincos_tables(int32_t sin512[512], int32_t cos512[512])
{
    if (!sin512 || !cos512)
        return GPSBB_E_BADARG;
    return make_sincos(sin512, cos512) ? GPSBB_OK : GPSBB_E_INTERNAL;
}

static void chain_only_free(gpsbb *h);

extern "C" void gpsbb_destroy(gpsbb_t *h)
{
    if (!h)
        return;
    (void)hipSetDevice(h->device);
    if (h->scratch)
        gpsbb_batch_destroy(h->scratch);
    release_all(h->h_fill, h->h_bounce);
    for (const gpsbb::HostReg &r : h->host_regs)
        (void)hipHostUnregister(r.host);
    h->host_regs.clear();
    chain_only_free(h);
    (void)drain_streams(h);
    release_all(h->d_tabs, h->d_ca, h->d_status, h->d_hz, h->d_clip, h->d_noise_tab, h->d_nclip);
    release_all(h->d_pack, h->d_level, h->d_digest, h->d_acq_chips, h->d_acq_rows, h->d_acq_grid, h->d_trk, h->d_fir, h->d_psd_tab, h->d_psd, h->d_exc, h->d_blank);
    release_all(h->acq_tm, h->trk_tm, h->fir_tm, h->psd_tm, h->exc_tm, h->blank_tm);
    delete h->pool;
    h->pool = nullptr;
    for_each_stream(h, [](hipStream_t st) { (void)hipStreamDestroy(st); });
    delete h;
}

static hipError_t create_seed_stream(hipStream_t *st);

/* Zero device memory NOW.  The library's streams are non-blocking ones: nothing orders them behind the null stream, and a
 * hipMemset of device memory returns before it has happened — a kernel launched afterwards on one of those streams can run
 * first and have its result wiped (found by the node driver's stress, tools/stress_node.py: four handles on one GPU, the
 * cleared carry of a fresh stream landing after the first push's fix-up had written it — every later block of the shard off
 * by that push's phase, once in a hundred runs).  So: on a stream of the handle, and waited for. */
#ifdef GPSBB_EXPERIMENTS
/* the ordering test's helper: one lane that keeps its stream busy for `ticks` of the 100 MHz wall clock */
__global__ void k_park(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks)
        __builtin_amdgcn_s_sleep(64);
}
#endif

static hipError_t zero_now(gpsbb *h, void *ptr, size_t bytes)
{
#ifdef GPSBB_EXPERIMENTS
    {
        /* The deterministic version of the race of round 4 (tests/test_laps_gpu.py::test_the_null_stream_owns_nothing):
         * GPSBB_X_PARK_NULL_MS=<ms> parks a kernel on the NULL stream before every zeroing — whatever the library still put on the
         * null stream, or ordered behind it, then lands that many milliseconds later than the code around it assumes, every time
         * instead of once in a hundred runs under load; GPSBB_X_NULL_MEMSET brings round 3's bug back (the zeroing as a null-stream
         * memset nobody waits for), so that the test can be seen to fail on it. */
        const long park = GPSBB_KNOB_LONG("GPSBB_X_PARK_NULL_MS", 0);
        if (park > 0)
            hipLaunchKernelGGL(k_park, dim3(1), dim3(1), 0, nullptr, (unsigned long long)park * 100000ull);
        if (GPSBB_KNOB_SET("GPSBB_X_NULL_MEMSET"))
            return hipMemsetAsync(ptr, 0, bytes, nullptr);
    }
#endif
    const hipError_t e = hipMemsetAsync(ptr, 0, bytes, h->s_seed);
    return e != hipSuccess ? e : hipStreamSynchronize(h->s_seed);
}

struct SynthKernel {
    void (*fn)(BatchDev, int16_t *);
    int lds; /* dynamic LDS bytes */
};
static const SynthKernel &synth_kernel(int variant, bool digest, int g);

extern "C" int gpsbb_create(gpsbb_t **out, int device)
{
    if (!out)
        return GPSBB_E_BADARG;
    *out = nullptr;
    /* The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), a new stream onto a queue of its own
     * while there is one left, and streams that share a queue run one after the other.  The steady state of a chained ring in
     * HBM keeps three streams of the handle busy — synthesis and two pre-passes, created here, first — which with the
     * process's null stream is that default.  A ring with host-bound output adds the copy stream: a host that runs one
     * exports GPU_MAX_HW_QUEUES=5 or more before its first HIP call.  The library itself neither reads
     * nor writes the environment. */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return GPSBB_E_NODEVICE;

    int32_t tabs[1024];
    if (!make_sincos(tabs + 512, tabs)) /* device layout: cos first, then sin */
        return GPSBB_E_INTERNAL;
    std::vector<uint32_t> ca(33 * 32, 0u);
    for (int prn = 1; prn <= 32; prn++) {
        uint8_t chips[GPSBB_CA_LEN];
        make_ca(prn, chips);
        for (int i = 0; i < GPSBB_CA_LEN; i++)
            if (chips[i])
                ca[prn * 32 + (i >> 5)] |= 1u << (i & 31);
    }

    gpsbb *h = new (std::nothrow) gpsbb;
    if (!h)
        return GPSBB_E_NOMEM;
    h->device = device;
    auto fail = [&](hipError_t e) {
        h->last_hip = (int)e;
        gpsbb_destroy(h);
        return e == hipErrorOutOfMemory ? GPSBB_E_NOMEM : GPSBB_E_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail(e);
    h->sm_count = prop.multiProcessorCount;
    if ((e = create_seed_stream(&h->s_seed)) != hipSuccess) return fail(e);
    {
        /* (experiments: GPSBB_SYNTH_STREAM_PRIO = p gives the synthesis streams queue priority p — HIP: -1 high, 0 normal, 1 low —,
         * GPSBB_SEED_STREAM_PRIO the pre-pass streams: whose workgroup gets a CU that has just come free) */
        const long sp = GPSBB_KNOB_LONG("GPSBB_SYNTH_STREAM_PRIO", 0);
        if (sp != 0) {
            if ((e = hipStreamCreateWithPriority(&h->s_compute, hipStreamNonBlocking, (int)sp)) != hipSuccess) return fail(e);
        } else {
            if ((e = hipStreamCreateWithFlags(&h->s_compute, hipStreamNonBlocking)) != hipSuccess) return fail(e);
        }
    }
    if ((e = create_seed_stream(&h->s_more[0])) != hipSuccess) return fail(e);
    if ((e = (hipError_t)h->d_tabs.reserve(sizeof tabs / sizeof tabs[0])) != hipSuccess) return fail(e);
    if ((e = (hipError_t)h->d_ca.reserve(ca.size())) != hipSuccess) return fail(e);
    if ((e = (hipError_t)h->d_status.reserve(1)) != hipSuccess) return fail(e);
    if ((e = (hipError_t)h->d_hz.reserve(8)) != hipSuccess) return fail(e);
    if ((e = (hipError_t)h->d_clip.reserve(1)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(h->d_tabs.p, tabs, sizeof tabs, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(h->d_ca.p, ca.data(), ca.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return fail(e); /* (the tables are there before any non-blocking stream runs) */
    h->h_ca = ca;
    if ((e = zero_now(h, h->d_status.p, 4)) != hipSuccess) return fail(e);
    if ((e = zero_now(h, h->d_hz.p, h->d_hz.cap * sizeof *h->d_hz.p)) != hipSuccess) return fail(e);
    if ((e = zero_now(h, h->d_clip.p, 8)) != hipSuccess) return fail(e);
    /* the synthesis kernels carve 76 - 156 KB of dynamic LDS per workgroup: above the 64 KB default limit */
    for (int v = GPSBB_VARIANT_SYNTH; v <= GPSBB_VARIANT_EV_FIXED; v++)
        for (int dg = 0; dg < 2; dg++)
            for (int g = 0; g <= EV_STATE_LOG2_MAX; g++) {
                const SynthKernel &k = synth_kernel(v, dg != 0, g);
                if (k.fn && (e = hipFuncSetAttribute(reinterpret_cast<const void *>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     k.lds)) != hipSuccess) return fail(e);
            }
    *out = h;
    return GPSBB_OK;
}

/* the instance of k_lap_pass2 (kind NCO_CODE / NCO_CARR) or k_lap_pass2_2 (kind -1: both) for a state granule of 2^g tiles */
typedef void (*LapKernelFn)(BatchDev, LapDev);
static LapKernelFn lap_pass2_kernel(int kind, bool wide, int g)
{
#define GPSBB_P2(W) {{k_lap_pass2<NCO_CODE, W, 0>, k_lap_pass2<NCO_CODE, W, 1>, k_lap_pass2<NCO_CODE, W, 2>}, \
                     {k_lap_pass2<NCO_CARR, W, 0>, k_lap_pass2<NCO_CARR, W, 1>, k_lap_pass2<NCO_CARR, W, 2>}, \
                     {k_lap_pass2_2<W, 0>, k_lap_pass2_2<W, 1>, k_lap_pass2_2<W, 2>}}
    static const LapKernelFn k[2][3][EV_STATE_LOG2_MAX + 1] = {GPSBB_P2(false), GPSBB_P2(true)};
#undef GPSBB_P2
    static_assert(NCO_CODE == 0 && NCO_CARR == 1, "lap_pass2_kernel's table");
    return k[wide ? 1 : 0][kind < 0 ? 2 : kind][g];
}

/* The synthesis kernels by GPSBB_VARIANT_*, without / with the blocks' digests fused, for a state granule of 2^g tiles (k_synth_ev
 * alone has instances beyond g = 0); fn null: no such instance. */
static const SynthKernel &synth_kernel(int variant, bool digest, int g)
{
#define GPSBB_SK(v, k) {k, synth_lds(v)}
#define GPSBB_SK1(v, k) {GPSBB_SK(v, k), {}, {}}
    static const SynthKernel k[GPSBB_VARIANT_EV_FIXED + 1][2][EV_STATE_LOG2_MAX + 1] = {
        {},
        {GPSBB_SK1(GPSBB_VARIANT_SYNTH, k_synth), {}},
        {{GPSBB_SK(GPSBB_VARIANT_EV, k_synth_ev<0>), GPSBB_SK(GPSBB_VARIANT_EV, k_synth_ev<1>), GPSBB_SK(GPSBB_VARIANT_EV, k_synth_ev<2>)},
         {GPSBB_SK(GPSBB_VARIANT_EV, k_synth_ev_digest<0>), GPSBB_SK(GPSBB_VARIANT_EV, k_synth_ev_digest<1>),
          GPSBB_SK(GPSBB_VARIANT_EV, k_synth_ev_digest<2>)}},
        {GPSBB_SK1(GPSBB_VARIANT_EV_DENSE, k_synth_ev_dense), {}},
        {GPSBB_SK1(GPSBB_VARIANT_PD_WIDE, k_synth_pd<true>), GPSBB_SK1(GPSBB_VARIANT_PD_WIDE, (k_synth_pd<true, true>))},
        {GPSBB_SK1(GPSBB_VARIANT_PD_NARROW, k_synth_pd<false>), GPSBB_SK1(GPSBB_VARIANT_PD_NARROW, (k_synth_pd<false, true>))},
        {GPSBB_SK1(GPSBB_VARIANT_EV_FIXED, k_synth_ev_fixed), {}},
    };
#undef GPSBB_SK1
#undef GPSBB_SK
    static_assert(GPSBB_VARIANT_SYNTH == 1 && GPSBB_VARIANT_EV == 2 && GPSBB_VARIANT_EV_DENSE == 3 && GPSBB_VARIANT_PD_WIDE == 4 &&
                      GPSBB_VARIANT_PD_NARROW == 5 && GPSBB_VARIANT_EV_FIXED == 6 && EV_STATE_LOG2_MAX == 2, "synth_kernel's table");
    return k[variant][digest ? 1 : 0][g];
}

/* upload `bytes` from pageable `src` through the batch's pinned arena (grown at the start of a set-up) */
static hipError_t stage_upload(gpsbb_batch *b, void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    const size_t at = (b->stage_used + 63) & ~(size_t)63;
    if (at + bytes > b->stage.cap) /* cannot happen: the arena was sized for this set-up */
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    memcpy(b->stage.p + at, src, bytes);
    b->stage_used = at + bytes;
    return hipMemcpyAsync(dst, b->stage.p + at, bytes, hipMemcpyHostToDevice, stream);
}

/* ---- batch set-up: plan, then stage ---------------------------------------------------------------- */

/* The pinned arena of one set-up's uploads, with room to spare: descriptors, plans, per-channel constants, chain scratch. */
static int stage_arena(gpsbb_batch *b, size_t nbc)
{
    gpsbb *h = b->h;
    const size_t need = nbc * (sizeof(gpsbb_chan_t) + sizeof(EvConst) + 8 + 2 * 4 + 5 * 4 +
                               (size_t)CHAIN_SEG_MAX * (sizeof(ChainDesc) + 8 + 8 + 2 * 4)) + 64 * 1024;
    if (b->upload_done) /* the previous set-up's copies out of the arena are long done; make sure */
        HIPCHK(h, hipEventSynchronize(b->upload_done));
    PUSH_MARK("arena");
    HIPCHK(h, (hipError_t)b->stage.reserve(need, need / 4));
    b->stage_used = 0;
    return GPSBB_OK;
}

/* Device scratch of every table set in use, sized here so that a launch never allocates (growing frees, and a free
 * synchronises the device), and the uploads of the plan's images on upload_stream. */
static int stage_plan(gpsbb_batch *b, hipStream_t upload_stream)
{
    gpsbb *h = b->h;
    const BatchPlan &pl = b->plan;
    const PlanImages &img = b->img;
    const size_t nbc = (size_t)pl.nblocks * pl.nch, nvbc = nbc * (size_t)pl.nseg;
    const bool room = b->max_sets == 1; /* a ring slot, whose pushes see different Dopplers (DevBuf::reserve) */
    HIPCHK(h, (hipError_t)b->d_ch.reserve(nbc));
    HIPCHK(h, (hipError_t)b->d_row_off.reserve(nbc + nvbc + 1));
    HIPCHK(h, (hipError_t)b->d_tile_ctr.reserve((size_t)NSETS * ((size_t)pl.nblocks + 1))); /* one set of counters per table set: a block's next tile, [nblocks] the helpers' tickets (ev_pick_block) */
    for (int set = 0; set < pl.nsets; set++) {
        TableSet &ts = b->sets[set];
        HIPCHK(h, (hipError_t)ts.end.reserve(nbc));
        if (pl.ev) {
            HIPCHK(h, (hipError_t)ts.tile_x.reserve(2 * nbc * (size_t)pl.nstates));
            HIPCHK(h, (hipError_t)ts.tile_nav.reserve(nbc * (size_t)pl.nstates));
            HIPCHK(h, (hipError_t)ts.rows.reserve(pl.total_rows + 4, room ? (size_t)(pl.total_rows / 2) : 0));
            HIPCHK(h, (hipError_t)ts.row_cnt.reserve(nbc + nvbc));
        } else {
            HIPCHK(h, (hipError_t)ts.rows.reserve(pl.total_rows + 4)); /* + slack: k_synth prefetches one row past a chain */
            HIPCHK(h, (hipError_t)ts.tile_row.reserve(2 * nbc * ((size_t)pl.ntiles + 1)));
            HIPCHK(h, (hipError_t)ts.row_cnt.reserve(2 * nbc));
        }
    }
    if (pl.ev) {
        HIPCHK(h, (hipError_t)b->d_evc.reserve(nbc));
        HIPCHK(h, stage_upload(b, b->d_evc.p, img.h_evc.data(), nbc * sizeof(EvConst), upload_stream));
    }
    if (pl.flags & GPSBB_FIXED_CARRIER) {
        HIPCHK(h, (hipError_t)b->d_kph0.reserve(nbc));
        HIPCHK(h, (hipError_t)b->d_kstep.reserve(nbc));
        HIPCHK(h, stage_upload(b, b->d_kph0.p, img.h_kph0.data(), nbc * 4, upload_stream));
        HIPCHK(h, stage_upload(b, b->d_kstep.p, img.h_kstep.data(), nbc * 4, upload_stream));
    }
    if (pl.laps) /* the lap-parallel pre-pass: scratch per table set */
        for (int set = 0; set < pl.nsets; set++)
            HIPCHK(h, (hipError_t)b->sets[set].lap.reserve(nbc, (size_t)pl.nch, (size_t)pl.nblocks, (size_t)pl.lap_chunk0[1][pl.nch], room));
    if (pl.chain_dev && !pl.laps) {
        /* the chain's scratch (ChainAux) needs no initial image: every field is written by the pass that owns it */
        for (int set = 0; set < pl.nsets; set++) {
            HIPCHK(h, (hipError_t)b->sets[set].aux.reserve(nvbc));
            if (!pl.chain_starts)
                HIPCHK(h, (hipError_t)b->sets[set].prefix.reserve(nvbc * (size_t)CHAIN_PREFIX_CAP));
        }
        HIPCHK(h, (hipError_t)b->d_cd.reserve(nvbc));
        HIPCHK(h, (hipError_t)b->d_start0.reserve(nvbc));
        /* one set of flags per table set: runs of a resident batch overlap, each on its own table set */
        HIPCHK(h, b->fix.reserve((size_t)NSETS * GPSBB_MAX_CHAN * pl.fix_chunks, upload_stream));
        HIPCHK(h, stage_upload(b, b->d_cd.p, img.h_cd.data(), nvbc * sizeof(ChainDesc), upload_stream));
        HIPCHK(h, stage_upload(b, b->d_start0.p, img.h_start0.data(), nvbc * sizeof(double), upload_stream));
    }
    PUSH_MARK("aux");
    HIPCHK(h, stage_upload(b, b->d_ch.p, img.h_ch.data(), nbc * sizeof(gpsbb_chan_t), upload_stream));
    PUSH_MARK("up_ch");
    if (!pl.laps) {
        HIPCHK(h, stage_upload(b, b->d_row_off.p, img.row_off.data(), (nbc + nvbc + 1) * 8, upload_stream));
        HIPCHK(h, (hipError_t)b->d_seed_order.reserve(img.h_seed_order.size()));
        HIPCHK(h, stage_upload(b, b->d_seed_order.p, img.h_seed_order.data(), img.h_seed_order.size() * 4, upload_stream));
        if (pl.chain_starts) {
            HIPCHK(h, (hipError_t)b->d_chain_order.reserve(img.h_chain_order.size()));
            HIPCHK(h, stage_upload(b, b->d_chain_order.p, img.h_chain_order.data(), img.h_chain_order.size() * 4, upload_stream));
        }
    }
    HIPCHK(h, b->upload_done.make(hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(b->upload_done, upload_stream));
    b->upload_stream = upload_stream;
    return GPSBB_OK;
}

/* Set a batch up for its descriptors: plan (plan_batch, or plan_finish behind a plan_begin the caller has run into `begun` and the
 * batch's images), then stage.  A plan that fails leaves the batch's plan as it was. */
static int batch_setup(gpsbb_batch *b, const PlanIn &in, const PlanOpts &o, hipStream_t upload_stream, const BatchPlan *begun = nullptr)
{
    BatchPlan pl;
    if (begun) {
        pl = *begun;
        plan_finish(pl, b->img, in, o, b->link);
    } else {
        const int rc = plan_batch(pl, b->img, in, o, b->link);
        if (rc != GPSBB_OK)
            return rc;
    }
    b->plan = pl;
    int rc = stage_arena(b, (size_t)in.nblocks * in.nch);
    rc = rc != GPSBB_OK ? rc : stage_plan(b, upload_stream);
    if (rc == GPSBB_OK)
        b->ran = false;
    return rc;
}

static gpsbb_batch *batch_new(gpsbb *h)
{
    gpsbb_batch *b = new (std::nothrow) gpsbb_batch;
    if (!b)
        return nullptr;
    b->h = h;
    b->seed_stream = h->s_seed;
    return b;
}

/* A stream for pre-pass kernels.  Experiments build: GPSBB_SEED_CUS = n confines it to n compute units (every
 * GPSBB_SEED_CU_STRIDE-th bit of the CU mask, default 1), to see what the pre-pass kernels' presence on a CU costs the
 * synthesis kernel there. */
static hipError_t create_seed_stream(hipStream_t *st)
{
    const long ncu = GPSBB_KNOB_LONG("GPSBB_SEED_CUS", 0);
    if (ncu > 0) {
        const long stride = std::max(1L, GPSBB_KNOB_LONG("GPSBB_SEED_CU_STRIDE", 1));
        const long first = GPSBB_KNOB_LONG("GPSBB_SEED_CU_FIRST", 0);
        uint32_t mask[16] = {0};
        for (long k = 0; k < ncu; k++) {
            const long bit = first + k * stride;
            if (bit < 512)
                mask[bit >> 5] |= 1u << (bit & 31);
        }
        return hipExtStreamCreateWithCUMask(st, 16, mask);
    }
    {
        const long pp = GPSBB_KNOB_LONG("GPSBB_SEED_STREAM_PRIO", 0);
        if (pp != 0)
            return hipStreamCreateWithPriority(st, hipStreamNonBlocking, (int)pp);
    }
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}

/* pre-pass stream k of the handle (0 = s_seed, 1 = s_more[0]: both from gpsbb_create; further ones on first use) */
static hipError_t seed_stream_at(gpsbb *h, unsigned k, hipStream_t *out)
{
    if (k == 0 || k >= (unsigned)SEED_STREAMS_MAX) {
        *out = h->s_seed;
        return hipSuccess;
    }
    hipStream_t &st = h->s_more[k - 1];
    if (!st) {
        hipError_t e = create_seed_stream(&st);
        if (e != hipSuccess)
            return e;
    }
    *out = st;
    return hipSuccess;
}

/* every other batch (and every other slot of a ring) seeds on the handle's second stream */
static hipError_t use_second_seed_stream(gpsbb_batch *b)
{
    return seed_stream_at(b->h, 1, &b->seed_stream);
}

/* The pre-pass stream of a batch's NEXT launch; the set-up of that launch uploads on the same stream, ahead of the pre-pass,
 * so neither waits for an event of the other.  Consecutive launches that may overlap take the handle's two pre-pass streams in
 * turn, so that two pre-passes are in flight beside the synthesis:
 *  - a batch with three or more table sets: run by run (two streams however many sets: a third pre-pass in flight bought nothing,
 *    tools/sweep_seed_streams.sh, and would want a fifth hardware queue);
 *  - a stream's slot with the device-side chain (b->link.d_carry set by the push, one table set): push by push (a pre-pass is a chain
 *    of latency-bound kernels, and the ring delivers one push per (that / streams));
 *  - anything else: the stream the batch was given when it was created (every other batch, every other slot). */
static hipError_t batch_prepass_stream(gpsbb_batch *b, bool chain_on_device, hipStream_t *out)
{
    gpsbb *h = b->h;
    *out = b->one_stream ? h->s_compute : b->seed_stream;
    if (b->one_stream)
        return hipSuccess;
    if (b->plan.nsets > 2) {
        const unsigned base = b->seed_stream == h->s_seed ? 0u : 1u;
        return seed_stream_at(h, (base + b->run_count) % std::min((unsigned)(b->plan.nsets - 1), STREAM_SEED_STREAMS), out);
    }
    if (b->link.d_carry && chain_on_device) {
        const unsigned nseed = (unsigned)GPSBB_KNOB_LONG("GPSBB_STREAM_SEED_STREAMS", STREAM_SEED_STREAMS);
        return seed_stream_at(h, b->link.stream_turn % (nseed >= 1 && nseed <= (unsigned)SEED_STREAMS_MAX ? nseed : STREAM_SEED_STREAMS), out);
    }
    return hipSuccess;
}

extern "C" void gpsbb_batch_destroy(gpsbb_batch_t *b)
{
    if (!b)
        return;
    (void)hipSetDevice(b->h->device);
    (void)drain_streams(b->h); /* its tables, its output and its events: pre-pass, synthesis and copy streams may all hold work on them */
    release_all(b->d_ch, b->d_row_off, b->upload_done);
    for (TableSet &ts : b->sets)
        ts.release();
    release_all(b->d_tile_ctr, b->d_seed_order, b->d_kph0, b->d_kstep, b->d_cd, b->d_start0, b->fix, b->d_chain_order, b->d_evc);
    release_all(b->hs_rows, b->hs_tile_row, b->hs_end, b->stage, b->hs_tile_x, b->hs_tile_nav);
    release_all(b->d_iq, b->d_dig, b->d_ds, b->d_ds_ctr, b->ds_tm);
    for (gpsbb_batch::Ev4 &t : b->evs)
        t.release();
    delete b;
}

extern "C" int gpsbb_batch_create(gpsbb_t *h, const gpsbb_chan_t *ch, int nblocks, int nch, double delt,
                                  int nsamp, unsigned flags, gpsbb_batch_t **out)
{
    if (!h || !out || (flags & (GPSBB_OUT_FORMAT_MASK | GPSBB_OUT_SHIFT_MASK))) /* a batch's output stays in HBM, as int16 */
        return GPSBB_E_BADARG;
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    gpsbb_batch *b = batch_new(h);
    if (!b)
        return GPSBB_E_NOMEM;
    if (h->batches_created++ & 1) { /* batches created one after the other seed side by side */
        const hipError_t e2 = use_second_seed_stream(b);
        if (e2 != hipSuccess) {
            gpsbb_batch_destroy(b);
            h->last_hip = (int)e2;
            return e2 == hipErrorOutOfMemory ? GPSBB_E_NOMEM : GPSBB_E_HIP;
        }
    }
    int rc = batch_setup(b, PlanIn{ch, nblocks, nch, delt, nsamp, flags}, plan_opts(h, b->max_sets), b->seed_stream);
    if (rc != GPSBB_OK) {
        gpsbb_batch_destroy(b);
        return rc;
    }
    HIPCHK(h, hipStreamSynchronize(b->seed_stream));
    *out = b;
    return GPSBB_OK;
}

extern "C" size_t gpsbb_batch_iq_bytes(const gpsbb_batch_t *b)
{
    return b ? (size_t)b->plan.nblocks * (size_t)b->plan.nsamp * 4 : 0;
}

/* ---- seeding on the host --------------------------------------------------------------------------
 * k_seed takes as long as its longest chain (one lane walks one chain, ~2 us per row), whatever the number
 * of chains.  For a handful of blocks — the drop-in single-block call above all — a few host threads walk
 * the same chains with the same code (gpsbb_nco.h) an order of magnitude faster per row, and the tables
 * (a few MB) are uploaded instead.  Same rows, same tile index, same end states as the kernel writes. */
namespace {

struct HostRowSink {
    SynRow *rows;
    uint32_t cap, cnt;
    bool overflow;
    unsigned long long dwrd_oob, itable_512;
    const uint32_t *dwrd;
    uint32_t dbit;
    int32_t *tr;
    size_t tstride;
    int32_t tile_t, ntiles, wrap_pend;

    void row(int32_t n0, uint32_t nav, double x, double S, bool after_wrap)
    {
        const int32_t nt = (int32_t)(((int64_t)n0 + TILE - 1) / TILE);
        const int32_t lim = nt < ntiles ? nt : ntiles;
        const int32_t here = (int32_t)(cnt < cap ? cnt : cap);
        for (; tile_t < lim; tile_t++, tr += tstride) {
            *tr = (here - 1) | wrap_pend;
            wrap_pend = 0;
        }
        if (after_wrap) {
            if ((n0 & (TILE - 1)) == 0 && tile_t < ntiles) {
                *tr = here | wrap_pend;
                tr += tstride;
                tile_t++;
            }
            wrap_pend = (int32_t)0x80000000;
        }
        if (cnt < cap) {
            SynRow r;
            r.n0 = n0;
            if (dwrd) {
                r.nav = nav | dbit;
                r.x = x;
                r.S = S;
            } else {
                r.nav = 0;
                r.x = mul_rn(x, 512.0);
                r.S = mul_rn(S, 512.0);
            }
            rows[cnt] = r;
        } else {
            overflow = true;
        }
        cnt++;
    }
    void table_index_512() { itable_512++; }
    void nav_fetch(uint32_t nav)
    {
        if (nav_iword(nav) >= GPSBB_N_DWRD)
            dwrd_oob++;
        dbit = nav_bit(dwrd, nav) < 0 ? 0x80000000u : 0u;
    }
    void finish()
    {
        if (cnt > cap)
            cnt = cap;
        for (; tile_t <= ntiles; tile_t++, tr += tstride) {
            *tr = ((int32_t)cnt - 1) | wrap_pend;
            wrap_pend = 0;
        }
        SynRow r;
        r.n0 = INT32_MAX;
        r.nav = 0;
        r.x = 0.0;
        r.S = 0.0;
        rows[cnt] = r;
    }
};

/* one chain (kind 0 = code, 1 = carrier) of channel k = block*nch + i: what seed_code_chain /
 * seed_carr_chain / seed_carr_fixed do on the device.  Returns false on a row-pool overflow. */
bool host_seed_chain(const gpsbb_batch *b, int kind, size_t k, unsigned long long *dwrd_oob, unsigned long long *itable_512)
{
    const BatchPlan &pl = b->plan;
    const PlanImages &img = b->img;
    const gpsbb_chan_t &c = img.h_ch[k];
    gpsbb_chan_state_t &e = b->hs_end.p[k];
    const size_t nbc = (size_t)pl.nblocks * pl.nch;
    const bool fixed = (pl.flags & GPSBB_FIXED_CARRIER) != 0;
    if (c.prn <= 0) {
        if (kind == 0) {
            e.code_phase = 0.0;
            e.iword = e.ibit = e.icode = e.dataBit = e.codeCA = 0;
            e._pad = 0;
        } else {
            e.carr_phase = 0.0;
        }
        return true;
    }
    const size_t blk = k / (size_t)pl.nch, i = k % (size_t)pl.nch;
    if (kind == 1 && fixed) {
        e.carr_phase = (double)(uint32_t)(img.h_kph0[k] + (uint32_t)pl.nsamp * (uint32_t)img.h_kstep[k]);
        if (pl.ev) {
            /* k_synth_pd: the table index at every tile start, in closed form (what k_tiles writes on the device) */
            double *tx = b->hs_tile_x.p + (blk * (2 * (size_t)pl.nch) + 2 * i + 1) * (size_t)pl.ntiles;
            for (int t = 0; t < pl.ntiles; t++)
                tx[t] = fixed_tile_index(img.h_kph0[k], img.h_kstep[k], t);
        }
        return true;
    }
    if (pl.ev) {
        /* breakpoint kernel: tile-start states instead of rows (what k_seed<true> writes) */
        uint32_t nav = kind == 0 ? nav_pack(c.icode, c.ibit, c.iword) : 0u;
        TileSink sink = make_tile_sink(b->hs_tile_x.p, b->hs_tile_nav.p, pl.nch, pl.ntiles, (int)blk, (int)i, kind,
                                       kind == 0 ? c.dwrd : nullptr, nav, nullptr);
        if (kind == 0) {
            const double s = mul_rn(c.f_code, pl.delt);
            const double x = build_rows_f64<NCO_CODE>(c.code_phase, s, nav, pl.nsamp, sink);
            sink.finish();
            e.code_phase = x;
            e.iword = nav_iword(nav);
            e.ibit = nav_ibit(nav);
            e.icode = nav_icode(nav);
            e.dataBit = nav_bit(c.dwrd, nav);
            const int ci = (int)x;
            e.codeCA = (int)((b->h->h_ca[(size_t)c.prn * 32 + (ci >> 5)] >> (ci & 31)) & 1u) * 2 - 1;
            e._pad = 0;
        } else {
            const double s = mul_rn(c.f_carr, pl.delt);
            e.carr_phase = build_rows_f64<NCO_CARR>(c.carr_phase, s, nav, pl.nsamp, sink);
            sink.finish();
        }
        *itable_512 += sink.hz_local[0];
        *dwrd_oob += sink.hz_local[1];
        return true;
    }
    const size_t chain = (size_t)kind * nbc + k;
    HostRowSink sink;
    sink.rows = b->hs_rows.p + img.row_off[chain];
    sink.cap = (uint32_t)(img.row_off[chain + 1] - img.row_off[chain] - 1);
    sink.cnt = 0;
    sink.overflow = false;
    sink.dwrd_oob = 0;
    sink.itable_512 = 0;
    sink.dwrd = kind == 0 ? c.dwrd : nullptr;
    uint32_t nav = kind == 0 ? nav_pack(c.icode, c.ibit, c.iword) : 0u;
    sink.dbit = kind == 0 && nav_bit(c.dwrd, nav) < 0 ? 0x80000000u : 0u;
    sink.tr = b->hs_tile_row.p + (blk * ((size_t)pl.ntiles + 1)) * (2 * (size_t)pl.nch) + 2 * i + (size_t)kind;
    sink.tstride = 2 * (size_t)pl.nch;
    sink.tile_t = 0;
    sink.ntiles = pl.ntiles;
    sink.wrap_pend = 0;
    if (kind == 0) {
        const double s = mul_rn(c.f_code, pl.delt);
        const double x = build_rows_f64<NCO_CODE>(c.code_phase, s, nav, pl.nsamp, sink);
        sink.finish();
        e.code_phase = x;
        e.iword = nav_iword(nav);
        e.ibit = nav_ibit(nav);
        e.icode = nav_icode(nav);
        e.dataBit = nav_bit(c.dwrd, nav);
        const int ci = (int)x;
        e.codeCA = (int)((b->h->h_ca[(size_t)c.prn * 32 + (ci >> 5)] >> (ci & 31)) & 1u) * 2 - 1;
        e._pad = 0;
    } else {
        const double s = mul_rn(c.f_carr, pl.delt);
        e.carr_phase = build_rows_f64<NCO_CARR>(c.carr_phase, s, nav, pl.nsamp, sink);
        sink.finish();
    }
    *dwrd_oob += sink.dwrd_oob;
    *itable_512 += sink.itable_512;
    return !sink.overflow;
}

} /* namespace */

/* Build the tables of one run on host threads and queue their upload on the seeding stream. */
static int host_seed_run(gpsbb_batch *b, const TableSet &ts, hipStream_t stream)
{
    const BatchPlan &pl = b->plan;
    gpsbb *h = b->h;
    const size_t nbc = (size_t)pl.nblocks * pl.nch;
    const size_t tr_n = 2 * nbc * ((size_t)pl.ntiles + 1);
    const size_t tx_n = 2 * nbc * (size_t)pl.ntiles, tn_n = nbc * (size_t)pl.ntiles;
    if (pl.ev) {
        HIPCHK(h, (hipError_t)b->hs_tile_x.reserve(tx_n, tx_n / 4));
        HIPCHK(h, (hipError_t)b->hs_tile_nav.reserve(tn_n, tn_n / 4));
    } else {
        HIPCHK(h, (hipError_t)b->hs_rows.reserve(pl.total_rows + 4, (pl.total_rows + 4) / 4));
        HIPCHK(h, (hipError_t)b->hs_tile_row.reserve(tr_n, tr_n / 4));
    }
    HIPCHK(h, (hipError_t)b->hs_end.reserve(nbc, nbc / 4));
    const size_t nchains = 2 * nbc;
    if (!h->pool) {
        const unsigned hw = std::thread::hardware_concurrency();
        size_t n = hw ? hw : 4;
        n = n > 32 ? 32 : n;
        h->pool = new (std::nothrow) WorkPool(n - 1);
        if (!h->pool)
            return GPSBB_E_NOMEM;
    }
    const size_t nthr = nchains; /* one slot of results per job */
    std::vector<unsigned long long> oob(nthr, 0ull), i512(nthr, 0ull);
    std::vector<char> ok(nthr, 1);
    /* carrier chains first: they are the long ones */
    h->pool->run(nchains, [&](size_t j) {
        const int kind = j < nbc ? 1 : 0;
        if (!host_seed_chain(b, kind, j < nbc ? j : j - nbc, &oob[j], &i512[j]))
            ok[j] = 0;
    });
    for (size_t t = 0; t < nthr; t++) {
        h->host_dwrd_oob += oob[t];
        h->host_itable_512 += i512[t];
        if (!ok[t])
            return GPSBB_E_INTERNAL;
    }
    if (pl.ev) {
        HIPCHK(h, hipMemcpyAsync(ts.tile_x.p, b->hs_tile_x.p, tx_n * sizeof(double), hipMemcpyHostToDevice, stream));
        HIPCHK(h, hipMemcpyAsync(ts.tile_nav.p, b->hs_tile_nav.p, tn_n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(ts.rows.p, b->hs_rows.p, pl.total_rows * sizeof(SynRow), hipMemcpyHostToDevice, stream));
        HIPCHK(h, hipMemcpyAsync(ts.tile_row.p, b->hs_tile_row.p, tr_n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    }
    HIPCHK(h, hipMemcpyAsync(ts.end.p, b->hs_end.p, nbc * sizeof(gpsbb_chan_state_t), hipMemcpyHostToDevice, stream));
    return GPSBB_OK;
}

/* The launch plan of the batch's next run (skip: the measurement hook takes effect on it), or of any run as far as batch_dev reads it. */
static LaunchPlan batch_launch_plan(const gpsbb_batch *b, bool skip = false)
{
    return plan_launch(b->plan, LaunchIn{cu_count(b->h->sm_count), b->want_digest, b->link.d_carry != nullptr, skip}, launch_opts());
}

static BatchDev batch_dev(const gpsbb_batch *b, const TableSet &ts, const LaunchPlan &lp)
{
    const BatchPlan &pl = b->plan;
    const size_t set = (size_t)(&ts - b->sets);
    BatchDev p;
    memset(&p, 0, sizeof p); /* (every field has a value, also the ones a later round adds) */
    p.ch = b->d_ch.p;
    p.nblocks = pl.nblocks;
    p.nch = pl.nch;
    p.nsamp = pl.nsamp;
    p.ntiles = pl.ntiles;
    p.st_log2 = pl.st_log2;
    p.nstates = pl.nstates;
    p.delt = pl.delt;
    p.flags = pl.flags;
    p.tabs = b->h->d_tabs.p;
    p.ca_bits = b->h->d_ca.p;
    p.rows = reinterpret_cast<SynRow *>(ts.rows.p);
    p.row_off = b->d_row_off.p;
    p.tile_row = ts.tile_row.p;
    p.row_cnt = ts.row_cnt.p;
    p.tile_ctr = b->d_tile_ctr.p + set * ((size_t)pl.nblocks + 1);
    p.kph0 = (pl.flags & GPSBB_FIXED_CARRIER) ? b->d_kph0.p : nullptr;
    p.kstep = (pl.flags & GPSBB_FIXED_CARRIER) ? b->d_kstep.p : nullptr;
    p.end = ts.end.p;
    p.status = b->h->d_status.p;
    p.hazards = b->h->d_hz.p;
    p.digest = b->want_digest ? b->d_dig.p : nullptr;
    p.seed_order = b->d_seed_order.p;
    p.seed_lanes = lp.seed_lanes;
    p.ev = pl.ev ? 1 : 0;
    p.ev_chunk = lp.ev_chunk;
    p.pd_danger = lp.pd_danger;
    p.tile_x = ts.tile_x.p;
    p.tile_nav = ts.tile_nav.p;
    p.evc = b->d_evc.p;
    p.chain_dev = pl.chain_dev ? 1 : 0;
    p.chain_starts = pl.chain_starts ? 1 : 0;
    p.aux = pl.chain_dev ? ts.aux.p : nullptr;
    p.nseg = pl.nseg;
    p.seg_tiles = pl.seg_tiles;
    p.nvb = pl.nblocks * pl.nseg;
    p.fix_end = b->fix.end.p ? b->fix.end.p + set * GPSBB_MAX_CHAN * pl.fix_chunks : nullptr;
    p.fix_flag = b->fix.flag.p ? b->fix.flag.p + set * GPSBB_MAX_CHAN * pl.fix_chunks : nullptr;
    p.fix_epoch = b->fix.epoch;
    p.fix_chunks = pl.fix_chunks;
    p.model_start = pl.chain_model ? 1 : 0;
    p.cd = pl.chain_dev ? b->d_cd.p : nullptr;
    p.start0 = pl.chain_dev ? b->d_start0.p : nullptr;
    p.prefix_rows = pl.chain_dev && !pl.chain_starts ? ts.prefix.p : nullptr;
    p.carry = pl.chain_dev ? b->link.d_carry : nullptr;
    p.cont0_mask = pl.cont0_mask;
    p.lap_end = nullptr;
    return p;
}

/* what a LapDev holds besides its scratch (LapScratch::dev), for a batch of nbc block-channels */
static void lap_dev_plan(LapDev &L, const uint32_t chunk0[2][GPSBB_MAX_CHAN + 1], bool chained, size_t nbc)
{
    memcpy(L.chunk0, chunk0, sizeof L.chunk0);
    L.chained = chained ? 1 : 0;
    L.jitter = (uint32_t)GPSBB_KNOB_LONG("GPSBB_LAP_JITTER", 0);
    L.burst = GPSBB_KNOB_SET("GPSBB_LAP_NO_BURST") ? 0 : (int)GPSBB_KNOB_LONG("GPSBB_LAP_BURST_SHARE", LAP_BURST_SHARE);
    L.unit[NCO_CODE] = lap_unit(NCO_CODE, nbc);
    L.unit[NCO_CARR] = lap_unit(NCO_CARR, nbc);
}

static LapDev lap_dev(const gpsbb_batch *b, const TableSet &ts)
{
    const BatchPlan &pl = b->plan;
    LapDev L;
    ts.lap.dev(L);
    lap_dev_plan(L, pl.lap_chunk0, pl.chain_dev, (size_t)pl.nblocks * pl.nch);
    return L;
}

/* The lap-parallel pre-pass of one kind of chain (gpsbb_laps.hip.h): plan, reference walks, scan, true walks, repair. */
template <int KIND>
static void lap_chain_kind(hipStream_t ss, const BatchDev &p, const LapDev &L, int nch, LapKernelFn pass2)
{
    const unsigned chunks = L.chunk0[KIND][nch] - L.chunk0[KIND][0];
    hipLaunchKernelGGL(k_lap_plan<KIND>, dim3(nch), dim3(64), 0, ss, p, L);
    hipLaunchKernelGGL(k_lap_pass1<KIND>, dim3(chunks), dim3(LAP_WG), 0, ss, p, L);
    hipLaunchKernelGGL(k_lap_scan<KIND>, dim3(nch), dim3(64), 0, ss, p, L);
    hipLaunchKernelGGL(pass2, dim3(chunks), dim3(LAP_WG), 0, ss, p, L);
    hipLaunchKernelGGL(k_lap_repair<KIND>, dim3(nch), dim3(64), 0, ss, p, L);
}

/* ... of the chains of `kind` (NCO_CODE, NCO_CARR), or of both in one grid per step (kind -1: the *_2 kernels); pass2 is
 * lap_pass2_kernel's instance for that kind */
static void lap_chain_launch(hipStream_t ss, const BatchDev &p, const LapDev &L, int nch, int kind, LapKernelFn pass2)
{
    if (kind == NCO_CODE) {
        lap_chain_kind<NCO_CODE>(ss, p, L, nch, pass2);
    } else if (kind == NCO_CARR) {
        lap_chain_kind<NCO_CARR>(ss, p, L, nch, pass2);
    } else {
        const unsigned chunks = L.chunk0[NCO_CODE][nch] - L.chunk0[NCO_CODE][0] + (L.chunk0[NCO_CARR][nch] - L.chunk0[NCO_CARR][0]);
        hipLaunchKernelGGL(k_lap_plan2, dim3(2 * nch), dim3(64), 0, ss, p, L);
        hipLaunchKernelGGL(k_lap_pass1_2, dim3(chunks), dim3(LAP_WG), 0, ss, p, L);
        hipLaunchKernelGGL(k_lap_scan2, dim3(2 * nch), dim3(64), 0, ss, p, L);
        hipLaunchKernelGGL(pass2, dim3(chunks), dim3(LAP_WG), 0, ss, p, L);
        hipLaunchKernelGGL(k_lap_repair2, dim3(2 * nch), dim3(64), 0, ss, p, L);
    }
}

/* The carrier chain by the row walks (gpsbb_walk.hip.h): pass A over the first carr_lanes lanes of p's plan (the carrier chains:
 * they come first) and the prefix — unless pass B starts from the host's drift model of every segment's start (plan_segments:
 * chain_model) —, pass B (k_walk<pass_b>: 2 leaves rows, 3 the blocks' start phases only) over all p.seed_lanes, and the fix-up:
 * k_chain_fix_par in workgroups of fix_wg lanes, or (fix_wg 0) k_chain_fix, the blocks in order.  A stream: this push's prefix /
 * fix-up follow the ones of the push before (other seeding stream). */
static hipError_t walk_chain_launch(hipStream_t ss, const BatchDev &p, int carr_lanes, bool pass_a, int pass_b, int fix_wg,
                                    const CarryEvents &ce)
{
    hipError_t e;
    if (pass_a) {
        BatchDev pa = p;
        pa.seed_lanes = carr_lanes;
        hipLaunchKernelGGL(k_walk<1>, dim3((carr_lanes + GPSBB_WALK_WG - 1) / GPSBB_WALK_WG), dim3(GPSBB_WALK_WG), 0, ss, pa);
        if ((e = CarryEvents::wait(ss, ce.prefix)) != hipSuccess)
            return e;
        hipLaunchKernelGGL(k_chain_prefix, dim3(p.nch), dim3(PREFIX_WG), 0, ss, p);
        if ((e = CarryEvents::record(ss, ce.prefix)) != hipSuccess)
            return e;
    }
    const dim3 wg_all((p.seed_lanes + GPSBB_WALK_WG - 1) / GPSBB_WALK_WG);
    if (pass_b == 2)
        hipLaunchKernelGGL(k_walk<2>, wg_all, dim3(GPSBB_WALK_WG), 0, ss, p);
    else
        hipLaunchKernelGGL(k_walk<3>, wg_all, dim3(GPSBB_WALK_WG), 0, ss, p);
    if ((e = CarryEvents::wait(ss, ce.fix)) != hipSuccess)
        return e;
    if (fix_wg == 0)
        hipLaunchKernelGGL(k_chain_fix, dim3(1), dim3(64), 0, ss, p);
    else if (fix_wg == FIXP_WG_ALONE)
        hipLaunchKernelGGL(k_chain_fix_par<FIXP_WG_ALONE>, dim3(p.nch, p.fix_chunks), dim3(FIXP_WG_ALONE), 0, ss, p);
    else
        hipLaunchKernelGGL(k_chain_fix_par<FIXP_WG_BATCH>, dim3(p.nch, p.fix_chunks), dim3(FIXP_WG_BATCH), 0, ss, p);
    return CarryEvents::record(ss, ce.fix);
}

/* The timing events of this launch: seed start/end (pre-pass stream), synth start/end (synthesis stream). */
static int launch_events(gpsbb_batch *b, Event **ev)
{
    gpsbb *h = b->h;
    /* (the drop-in call's scratch batch, everything on one stream and waited for before the call returns: no events — each record
     * is a packet between two kernels, 5 us of nothing on a call of 140) */
    if (b->one_stream) {
        if (b->evs.empty())
            b->evs.emplace_back();
        b->ev_used = 0;
        *ev = b->evs[0].e;
        return GPSBB_OK;
    }
    if (b->ev_used == b->evs.size()) {
        if (b->evs.size() >= 4096) {
            b->ev_used = 0; /* wrap: only the most recent runs are kept */
        } else {
            gpsbb_batch::Ev4 t;
            for (Event &e : t.e) {
                const hipError_t rc = e.make(hipEventDefault);
                if (rc != hipSuccess)
                    t.release(); /* all four or none */
                HIPCHK(h, rc);
            }
            b->evs.push_back(t);
        }
    }
    *ev = b->evs[b->ev_used++].e;
    return GPSBB_OK;
}

/* The pre-pass of one run into table set `set`, on stream ss, as the launch plan says. */
static int prepass_launch(gpsbb_batch *b, int set, const BatchDev &p, const LaunchPlan &lp, hipStream_t ss)
{
    const BatchPlan &pl = b->plan;
    gpsbb *h = b->h;
    const TableSet &ts = b->sets[set];
    const CarryEvents ce = {b->link.d_carry ? b->link.ev_prefix : nullptr, b->link.d_carry ? b->link.ev_fix : nullptr};
    if (lp.chain) {
        /* the carrier chain by the row walks: over the seed order (rows for the model kernels), or over the chain order */
        BatchDev pw = p;
        if (lp.chain_order) {
            pw.seed_order = b->d_chain_order.p;
            pw.seed_lanes = lp.walk_lanes;
        }
        HIPCHK(h, walk_chain_launch(ss, pw, lp.carr_lanes, lp.pass_a, lp.pass_b, lp.fix_wg, ce));
    }
    switch (lp.prepass) {
    case PREPASS_SKIP:
        break;
    case PREPASS_HOST: {
        /* the previous user of the pinned images (this batch's last run) has been copied out: its upload was
         * followed by the synthesis kernel, which that set's synth_done_ref covers */
        const TableSet &prev = b->sets[(set + pl.nsets - 1) % pl.nsets];
        if (prev.synth_pending)
            HIPCHK(h, hipEventSynchronize(prev.synth_done_ref));
        return host_seed_run(b, ts, ss);
    }
    case PREPASS_LAPS: {
        /* plan, reference walks, scan, true walks, repair — the code chains first (nothing of theirs waits for another push), then
         * the carriers: a stream's push starts from the exact phase the push before it left on the device, so its plan follows
         * that push's repair kernel */
        const LapDev L = lap_dev(b, ts);
        if (!lp.lap_merged)
            lap_chain_launch(ss, p, L, pl.nch, NCO_CODE, lap_pass2_kernel(NCO_CODE, lp.lap_wide, lp.granule));
        if (lp.lap_fixed) {
            /* no chain to walk: the plan kernel leaves the end states, the tile states are a closed form */
            hipLaunchKernelGGL(k_lap_plan<NCO_CARR>, dim3(pl.nch), dim3(64), 0, ss, p, L);
            hipLaunchKernelGGL(k_lap_fixed_tiles, dim3(pl.nblocks * pl.nch), dim3(256), 0, ss, p);
        } else {
            const int kind = lp.lap_merged ? -1 : NCO_CARR;
            HIPCHK(h, ce.wait_both(ss));
            lap_chain_launch(ss, p, L, pl.nch, kind, lap_pass2_kernel(kind, lp.lap_wide, lp.granule));
            HIPCHK(h, ce.record_both(ss));
        }
        break;
    }
    case PREPASS_WALKS:
        if (!lp.chain)
            hipLaunchKernelGGL(k_walk<0>, dim3((lp.seed_lanes + GPSBB_WALK_WG - 1) / GPSBB_WALK_WG), dim3(GPSBB_WALK_WG), 0, ss, p);
        hipLaunchKernelGGL(k_tiles, dim3((1 + pl.nseg) * pl.nblocks * pl.nch), dim3(GPSBB_TILES_WG), 0, ss, p);
        break;
    case PREPASS_SEED: {
        const dim3 grid((lp.seed_lanes + GPSBB_SEED_WG - 1) / GPSBB_SEED_WG);
        if (lp.seed_ev)
            hipLaunchKernelGGL(k_seed<true>, grid, dim3(GPSBB_SEED_WG), 0, ss, p);
        else
            hipLaunchKernelGGL(k_seed<false>, grid, dim3(GPSBB_SEED_WG), 0, ss, p);
        break;
    }
    }
    return GPSBB_OK;
}

/* The synthesis kernel of one run on stream sc, and the blocks' digests behind it where no variant leaves them itself. */
static int synth_launch(gpsbb_batch *b, const BatchDev &p, const LaunchPlan &lp, hipStream_t sc, int16_t *d_iq)
{
    const SynthKernel &k = synth_kernel(lp.variant, lp.digest_fused, lp.granule);
    hipLaunchKernelGGL(k.fn, dim3(lp.grid_x, lp.grid_y), dim3(lp.wg), k.lds, sc, p, d_iq);
    if (lp.digest_gx)
        hipLaunchKernelGGL(k_block_digest, dim3(lp.digest_gx, lp.digest_gy), dim3(256), 0, sc, (const uint32_t *)d_iq, b->plan.nsamp, b->d_dig.p);
    HIPCHK(b->h, hipGetLastError());
    return GPSBB_OK;
}

/* One run of a batch: its timing events, the pre-pass on a pre-pass stream, the synthesis on a synthesis stream behind it. */
static int batch_launch(gpsbb_batch *b, int16_t *d_iq)
{
    const BatchPlan &pl = b->plan;
    gpsbb *h = b->h;
    const int set = (int)(b->run_count % (unsigned)pl.nsets);
    TableSet &ts = b->sets[set];
    b->fix.epoch++; /* a number no earlier launch of this batch handed to k_chain_fix_par */
    if (b->want_digest)
        HIPCHK(h, (hipError_t)b->d_dig.reserve((size_t)pl.nblocks));
    const LaunchPlan lp = batch_launch_plan(b, h->opt_skip_seed && b->run_count >= (unsigned)pl.nsets);
    const BatchDev p = batch_dev(b, ts, lp);
    const bool timed = !b->one_stream;
    Event *ev = nullptr;
    int rc = launch_events(b, &ev);
    if (rc != GPSBB_OK)
        return rc;
    PUSH_MARK("l_ev");

    /* The pre-pass runs on a seeding stream of its own: it may start as soon as the synthesis kernel that last
     * read this table set has finished, i.e. it overlaps the synthesis of the runs before it.  With three sets
     * consecutive runs take the handle's two seeding streams in turn, so that two pre-passes are in flight. */
    hipStream_t ss = nullptr;
    HIPCHK(h, batch_prepass_stream(b, pl.chain_dev, &ss));
    /* (a push's set-up uploaded on this very stream: in order already, and no wait packet ahead of the plan kernel) */
    if (b->upload_done && b->upload_stream != ss)
        HIPCHK(h, hipStreamWaitEvent(ss, b->upload_done, 0));
    if (ts.synth_pending)
        HIPCHK(h, hipStreamWaitEvent(ss, ts.synth_done_ref, 0));
    if (timed)
        HIPCHK(h, hipEventRecord(ev[0], ss));
    rc = prepass_launch(b, set, p, lp, ss);
    if (rc != GPSBB_OK)
        return rc;
    HIPCHK(h, hipGetLastError());
    if (timed)
        HIPCHK(h, hipEventRecord(ev[1], ss));
    h->last_prepass = lp.info_prepass;
    h->last_kernel = lp.last_kernel;
    h->last_variant = lp.variant;
    h->last_chain_dev = lp.last_chain_dev;
    PUSH_MARK("l_pre");

    /* off by default: +2 % on a stream of pushes, but overlapping kernels make the per-launch time (the roofline figure)
     * meaningless and re-runs of a resident batch get slower */
    const bool one_cs = !GPSBB_KNOB_SET("GPSBB_TWO_COMPUTE_STREAMS");
    /* consecutive launches take the two synthesis streams in turn — they work on different table sets (or, slots of
     * a ring, different batches) — except re-runs of a batch that has a single table set */
    hipStream_t sc = h->s_compute;
    if (!one_cs && !b->one_stream && (pl.nsets >= 2 || b->max_sets == 1) && ((h->compute_turn++) & 1u)) {
        if (!h->s_compute2)
            HIPCHK(h, hipStreamCreateWithFlags(&h->s_compute2, hipStreamNonBlocking));
        sc = h->s_compute2;
    }
    b->last_cs = sc;
    if (sc != ss)
        HIPCHK(h, hipStreamWaitEvent(sc, ev[1], 0));
    if (!lp.ctr_reset)
        HIPCHK(h, hipMemsetAsync(p.tile_ctr, 0, ((size_t)pl.nblocks + 1) * sizeof(int32_t), sc));
    if (timed)
        HIPCHK(h, hipEventRecord(ev[2], sc));
    if (b->want_digest)
        HIPCHK(h, hipMemsetAsync(b->d_dig.p, 0, (size_t)pl.nblocks * sizeof(unsigned long long), sc));
    rc = synth_launch(b, p, lp, sc, d_iq);
    if (rc != GPSBB_OK)
        return rc;
    if (timed)
        HIPCHK(h, hipEventRecord(ev[3], sc));
    /* the run's end-of-synthesis event doubles as "this table set is free again" and as what a stream's copy stream
     * waits for: every further record on the synthesis stream is another packet between two kernels */
    ts.synth_done_ref = ev[3];
    b->last_done = ev[3];
    ts.synth_pending = timed;
    b->last_set = set;
    b->run_count++;
    b->ran = true;
    return GPSBB_OK;
}

extern "C" int gpsbb_batch_run(gpsbb_batch_t *b, int16_t *d_iq)
{
    if (!b)
        return GPSBB_E_BADARG;
    gpsbb *h = b->h;
    HIPCHK(h, hipSetDevice(h->device));
    if (!d_iq) {
        HIPCHK(h, (hipError_t)b->d_iq.reserve((size_t)b->plan.nblocks * b->plan.nsamp * 2));
        d_iq = b->d_iq.p;
        b->last_iq = d_iq;
    } else {
        b->last_iq = nullptr;
        b->last_ext_iq = d_iq; /* gpsbb_batch_read copies from it for as long as the caller keeps it alive */
    }
    return batch_launch(b, d_iq);
}

extern "C" int16_t *gpsbb_batch_device_iq(gpsbb_batch_t *b) { return b ? b->last_iq : nullptr; }

extern "C" int gpsbb_sync(gpsbb_t *h)
{
    if (!h)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, drain_streams(h));
    uint32_t st = 0;
    HIPCHK(h, hipMemcpy(&st, h->d_status.p, 4, hipMemcpyDeviceToHost));
    if (st) {
        HIPCHK(h, zero_now(h, h->d_status.p, 4));
        return GPSBB_E_INTERNAL;
    }
    return GPSBB_OK;
}

extern "C" int gpsbb_batch_read(gpsbb_batch_t *b, int16_t *iq_out, gpsbb_chan_state_t *end_state)
{
    if (!b || !b->ran)
        return GPSBB_E_STATE;
    gpsbb *h = b->h;
    HIPCHK(h, hipSetDevice(h->device));
    if (iq_out) {
        const int16_t *src = b->last_iq ? b->last_iq : b->last_ext_iq;
        if (!src)
            return GPSBB_E_STATE;
        HIPCHK(h, hipMemcpy(iq_out, src, gpsbb_batch_iq_bytes(b), hipMemcpyDeviceToHost));
    }
    if (end_state)
        HIPCHK(h, hipMemcpy(end_state, b->sets[b->last_set].end.p, (size_t)b->plan.nblocks * b->plan.nch * sizeof(gpsbb_chan_state_t),
                            hipMemcpyDeviceToHost));
    return GPSBB_OK;
}

extern "C" int gpsbb_device_read(gpsbb_t *h, void *host_dst, const void *device_src, size_t bytes)
{
    if (!h || !host_dst || !device_src)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(host_dst, device_src, bytes, hipMemcpyDeviceToHost));
    return GPSBB_OK;
}

/* How every call that reads device IQ begins, once its arguments have passed: the device; then the work of every launch the
 * caller may be reading the output of is on this handle's streams, so wait for it (what follows goes on the synthesis stream,
 * ordered behind everything the handle rendered); then, for a call with noise, the knot table.  Returns a GPSBB_* code. */
static int iq_call_begin(gpsbb *h, bool noise);

/* both digest calls: k_block_digest over nblocks blocks at d_iq on `stream`, about wgs workgroups in all, and the sums copied out */
static int digest_blocks(gpsbb *h, hipStream_t stream, long wgs, const int16_t *d_iq, long nblocks, int nsamp, uint64_t *digest_out)
{
    HIPCHK(h, (hipError_t)h->d_digest.reserve((size_t)nblocks));
    HIPCHK(h, hipMemsetAsync(h->d_digest.p, 0, (size_t)nblocks * sizeof(unsigned long long), stream));
    /* enough workgroups per block to fill the chip however few blocks there are, never pieces below 4 KB */
    long chunks = (wgs + nblocks - 1) / nblocks;
    const long max_chunks = ((long)nsamp + 1023) / 1024;
    chunks = chunks > max_chunks ? max_chunks : (chunks < 1 ? 1 : chunks);
    hipLaunchKernelGGL(k_block_digest, dim3((unsigned)chunks, (unsigned)nblocks), dim3(256), 0, stream, (const uint32_t *)d_iq, nsamp, h->d_digest.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(digest_out, h->d_digest.p, (size_t)nblocks * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(h, hipStreamSynchronize(stream));
    return GPSBB_OK;
}

extern "C" int gpsbb_device_digest(gpsbb_t *h, const int16_t *d_iq, long nblocks, int nsamp, uint64_t *digest_out)
{
    if (!h || !d_iq || !digest_out || nblocks < 1 || nblocks > 65535 || nsamp < 1)
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, false);
    return rc != GPSBB_OK ? rc : digest_blocks(h, h->s_compute, 2048, d_iq, nblocks, nsamp, digest_out);
}

/* (no wait for the handle: a ring's slot is digested while the pushes behind it run) */
extern "C" int gpsbb_slot_digest(gpsbb_t *h, const int16_t *d_iq, long nblocks, int nsamp, uint64_t *digest_out)
{
    if (!h || !d_iq || !digest_out || nblocks < 1 || nblocks > 65535 || nsamp < 1)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->s_digest)
        HIPCHK(h, hipStreamCreateWithFlags(&h->s_digest, hipStreamNonBlocking));
    return digest_blocks(h, h->s_digest, GPSBB_KNOB_LONG("GPSBB_SLOT_DIGEST_WGS", 2048), d_iq, nblocks, nsamp, digest_out);
}

extern "C" int gpsbb_get_hazards(gpsbb_t *h, gpsbb_hazards_t *out, int reset)
{
    if (!h || !out)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long v[2];
    HIPCHK(h, hipMemcpy(v, h->d_hz.p, 16, hipMemcpyDeviceToHost));
    out->itable_512 = v[0];
    out->itable_512 += h->host_itable_512;
    out->dwrd_oob = v[1] + h->host_dwrd_oob;
    if (reset) {
        HIPCHK(h, zero_now(h, h->d_hz.p, 16));
        h->host_dwrd_oob = 0;
        h->host_itable_512 = 0;
    }
    return GPSBB_OK;
}

extern "C" int gpsbb_batch_last_timing(gpsbb_batch_t *b, float *ms_seed, float *ms_synth, float *ms_total)
{
    if (!b || !b->ran || b->ev_used == 0)
        return GPSBB_E_STATE;
    gpsbb *h = b->h;
    const Event *ev = b->evs[b->ev_used - 1].e;
    float a = 0, c = 0, t = 0;
    HIPCHK(h, hipEventElapsedTime(&a, ev[0], ev[1]));
    HIPCHK(h, hipEventElapsedTime(&c, ev[2], ev[3]));
    HIPCHK(h, hipEventElapsedTime(&t, ev[0], ev[3]));
    if (ms_seed) *ms_seed = a;
    if (ms_synth) *ms_synth = c;
    if (ms_total) *ms_total = t;
    return GPSBB_OK;
}

extern "C" int gpsbb_batch_timing_stats(gpsbb_batch_t *b, int *nruns, float *ms_seed_sum, float *ms_synth_sum,
                                        float *ms_total_sum, int reset)
{
    if (!b)
        return GPSBB_E_BADARG;
    gpsbb *h = b->h;
    float sa = 0, sc = 0, stt = 0;
    for (size_t k = 0; k < b->ev_used; k++) {
        const Event *ev = b->evs[k].e;
        float a = 0, c = 0, t = 0;
        HIPCHK(h, hipEventElapsedTime(&a, ev[0], ev[1]));
        HIPCHK(h, hipEventElapsedTime(&c, ev[2], ev[3]));
        HIPCHK(h, hipEventElapsedTime(&t, ev[0], ev[3]));
        sa += a;
        sc += c;
        stt += t;
    }
    if (nruns) *nruns = (int)b->ev_used;
    if (ms_seed_sum) *ms_seed_sum = sa;
    if (ms_synth_sum) *ms_synth_sum = sc;
    if (ms_total_sum) *ms_total_sum = stt;
    if (reset)
        b->ev_used = 0;
    return GPSBB_OK;
}

extern "C" int gpsbb_fill_ceiling(gpsbb_t *h, void *d_dst, size_t bytes, int iters, float *ms)
{
    if (!h || !d_dst || bytes < 16 || iters < 1 || !ms)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    Event e0, e1;
    const AtExit done{[&] { release_all(e0, e1); }};
    HIPCHK(h, e0.make(hipEventDefault));
    HIPCHK(h, e1.make(hipEventDefault));
    const size_t n16 = bytes / 16;
    const int grid = (int)cu_count(h->sm_count) * 8;
    hipLaunchKernelGGL(k_fill_ceiling, dim3(grid), dim3(256), 0, h->s_compute, (uint4 *)d_dst, n16, 1u);
    HIPCHK(h, hipEventRecord(e0, h->s_compute));
    for (int i = 0; i < iters; i++)
        hipLaunchKernelGGL(k_fill_ceiling, dim3(grid), dim3(256), 0, h->s_compute, (uint4 *)d_dst, n16, (uint32_t)i);
    HIPCHK(h, hipEventRecord(e1, h->s_compute));
    HIPCHK(h, hipEventSynchronize(e1));
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, e0, e1));
    *ms = t / iters;
    return GPSBB_OK;
}

/* ---- the synchronous single-block surface ------------------------------------------------------------ */

/* What the drop-in call waits for.  Everything of the call is ordered in front of the synthesis stream's tail (upload -> pre-pass
 * -> synthesis by events), so ONE stream is waited for, not the handle's ten; the end states and the status word come back
 * through pinned memory behind the IQ on that stream instead of as two blocking copies of their own (each a round trip of
 * 25 - 30 us: with the ten-kernel pre-pass they were half of the call's 0.26 ms for the reference's block). */
/* end states and status word into the handle's pinned page, written by the device: one launch behind the synthesis kernel
 * instead of two copies (each a packet of its own and 4 us of blit kernel) */
__global__ void k_fill_tail(const gpsbb_chan_state_t *end, const uint32_t *status, unsigned char *host, int nch, uint32_t *host_status)
{
    const uint32_t *src = reinterpret_cast<const uint32_t *>(end);
    uint32_t *dst = reinterpret_cast<uint32_t *>(host);
    const uint32_t words = end ? (uint32_t)nch * (uint32_t)(sizeof(gpsbb_chan_state_t) / 4) : 0u;
    for (uint32_t k = threadIdx.x; k < words; k += blockDim.x)
        dst[k] = src[k];
    if (threadIdx.x == 0)
        *host_status = *status;
}

/* ---- output formats (GPSBB_OUT_*) ---- */

/* The output format of `flags`: 0 = SC16, PACK_SC8 (with *shift), PACK_SC1; -1 for an unknown format, a shift on anything but SC8,
 * bits above the shift, SC1 with nsamp % 4 != 0 (GPSBB_E_BADARG).  The bits below the format are the caller's business. */
static int out_format(unsigned flags, long nsamp, int *shift)
{
    const unsigned f = (flags & GPSBB_OUT_FORMAT_MASK) >> 8, sh = (flags & GPSBB_OUT_SHIFT_MASK) >> 12;
    *shift = (int)sh;
    if ((flags >> 16) || nsamp < 1 || f > 2 || (sh && f != 1) || (f == 2 && nsamp % 4))
        return -1;
    return f == 1 ? PACK_SC8 : (f == 2 ? PACK_SC1 : 0);
}

static size_t out_block_bytes(int fmt, size_t nsamp) { return fmt == PACK_SC8 ? nsamp * 2 : (fmt == PACK_SC1 ? nsamp / 4 : nsamp * 4); }

extern "C" long gpsbb_out_bytes(unsigned flags, long nsamp)
{
    int shift;
    const int fmt = out_format(flags, nsamp, &shift);
    return fmt < 0 ? GPSBB_E_BADARG : (long)out_block_bytes(fmt, (size_t)nsamp);
}

struct ImpairCall;
static hipError_t out_launch(gpsbb *h, int fmt, int shift8, const ImpairCall *ic, const int16_t *src, void *dst, size_t n, hipStream_t stream);

extern "C" int gpsbb_device_pack(gpsbb_t *h, const int16_t *d_iq, long nblocks, int nsamp, unsigned flags, void *host_dst)
{
    int shift;
    const int fmt = out_format(flags, nsamp, &shift);
    if (!h || !d_iq || !host_dst || nblocks < 1 || nsamp < 1 || fmt < 0 || (flags & 0xffu))
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, false);
    if (rc != GPSBB_OK)
        return rc;
    const size_t bytes = (size_t)nblocks * out_block_bytes(fmt, (size_t)nsamp);
    if (fmt == 0) {
        HIPCHK(h, hipMemcpy(host_dst, d_iq, bytes, hipMemcpyDeviceToHost));
        return GPSBB_OK;
    }
    HIPCHK(h, (hipError_t)h->d_pack.reserve(bytes));
    HIPCHK(h, out_launch(h, fmt, shift, nullptr, d_iq, h->d_pack.p, (size_t)nblocks * (size_t)nsamp * 2, h->s_compute));
    HIPCHK(h, hipMemcpyAsync(host_dst, h->d_pack.p, bytes, hipMemcpyDeviceToHost, h->s_compute));
    HIPCHK(h, hipStreamSynchronize(h->s_compute));
    return GPSBB_OK;
}

/* ---- receiver noise (include/gpsbb.h gpsbb_noise_t; gpsbb_noise.hip.h) ---- */

/* Phi^-1(1 - q) for 0 < q < 1: Acklam's rational approximation, then one Halley step on erfc (double precision throughout) */
static double upper_quantile(double q)
{
    static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02,
                                -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01,
                                -1.328068155288572e+01};
    static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00,
                                4.374664141464968e+00, 2.938163982698783e+00};
    static const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
    const double p = q; /* x = Phi^-1(p); the answer is -x */
    double x;
    if (p < 0.02425) {
        const double r = std::sqrt(-2.0 * std::log(p));
        x = (((((c[0] * r + c[1]) * r + c[2]) * r + c[3]) * r + c[4]) * r + c[5]) / ((((d[0] * r + d[1]) * r + d[2]) * r + d[3]) * r + 1.0);
    } else if (p <= 1.0 - 0.02425) {
        const double r0 = p - 0.5, r = r0 * r0;
        x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * r0 /
            (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
    } else {
        const double r = std::sqrt(-2.0 * std::log(1.0 - p));
        x = -(((((c[0] * r + c[1]) * r + c[2]) * r + c[3]) * r + c[4]) * r + c[5]) / ((((d[0] * r + d[1]) * r + d[2]) * r + d[3]) * r + 1.0);
    }
    for (int k = 0; k < 2; k++) {
        const double e = 0.5 * std::erfc(-x / std::sqrt(2.0)) - p;
        const double u = e * std::sqrt(2.0 * M_PI) * std::exp(x * x / 2.0);
        x = x - u / (1.0 + x * u / 2.0);
    }
    return -x;
}

/* the knots K of step 2 (include/gpsbb.h), computed once */
static const int32_t *noise_knots()
{
    static int32_t k[NOISE_KNOTS];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int i = 0; i < NOISE_KNOTS; i++) {
            double t;
            if (i < 128) {
                t = (double)i;
            } else {
                const int e = i / 64 + 5;
                t = std::ldexp(1.0, e) + (double)(i % 64) * std::ldexp(1.0, e - 6);
            }
            k[i] = (int32_t)std::llround(65536.0 * upper_quantile((t + 0.5) / 4294967296.0));
        }
    });
    return k;
}

extern "C" int gpsbb_noise_table(int32_t *knots, int cap)
{
    const int32_t *k = noise_knots();
    if (knots)
        for (int i = 0; i < cap && i < NOISE_KNOTS; i++)
            knots[i] = k[i];
    return NOISE_KNOTS;
}

extern "C" double gpsbb_noise_sigma(double cn0_dbhz, double gain, double delt)
{
    if (!std::isfinite(cn0_dbhz) || !(gain > 0.0) || !std::isfinite(gain) || !(delt > 0.0) || !std::isfinite(delt))
        return NAN;
    int32_t s[512], c[512];
    if (!make_sincos(s, c))
        return NAN;
    double p1 = 0.0;
    for (int i = 0; i < 512; i++)
        p1 += (double)c[i] * c[i] + (double)s[i] * s[i];
    p1 /= 512.0;
    return std::sqrt(p1 * gain * gain / delt / (2.0 * std::pow(10.0, cn0_dbhz / 10.0)));
}

/* a gpsbb_noise_t the library takes, turned into the kernel's arguments; false: GPSBB_E_BADARG */
static bool noise_args(const gpsbb_noise_t *nz, NoiseArgs *a)
{
    if (!(nz->sigma > 0.0) || !(nz->sigma <= 1048576.0) || nz->shift < 0 || nz->shift > 7)
        return false;
    a->key0 = (uint32_t)nz->seed;
    a->key1 = (uint32_t)(nz->seed >> 32);
    a->sample0 = nz->sample0;
    a->s256 = (int)std::llround(256.0 * nz->sigma);
    a->shift = nz->shift;
    a->shift8 = 0;
    return true;
}

/* the knot table on the device and the clip counter: made on the handle's first call with noise */
static hipError_t noise_ready(gpsbb *h)
{
    if (h->d_noise_tab.p)
        return hipSuccess;
    const int32_t *k = noise_knots();
    std::vector<int2> t(NOISE_KNOTS - 1);
    for (int i = 0; i + 1 < NOISE_KNOTS; i++)
        t[i] = make_int2(k[i], k[i + 1] - k[i]);
    hipError_t e = (hipError_t)h->d_nclip.reserve(1);
    if (e == hipSuccess) e = zero_now(h, h->d_nclip.p, 8);
    if (e == hipSuccess) e = (hipError_t)h->d_noise_tab.reserve(t.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_noise_tab.p, t.data(), t.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr); /* (the table is there before any non-blocking stream reads it) */
    if (e != hipSuccess)
        release_all(h->d_noise_tab, h->d_nclip); /* both or neither (FixScratch::reserve): the next call with noise starts clean */
    return e;
}

static int iq_call_begin(gpsbb *h, bool noise)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = gpsbb_sync(h);
    if (rc != GPSBB_OK)
        return rc;
    if (noise)
        HIPCHK(h, noise_ready(h));
    return GPSBB_OK;
}

extern "C" int gpsbb_device_noise(gpsbb_t *h, const int16_t *d_src, int16_t *d_dst, long nblocks, int nsamp, const gpsbb_noise_t *nz)
{
    if (!nz)
        return GPSBB_E_BADARG;
    return gpsbb_device_impair(h, d_src, d_dst, nblocks, nsamp, nz, nullptr);
}

/* ---- interference (include/gpsbb.h gpsbb_interf_t; gpsbb_interf.h, gpsbb_interf.hip.h) ---- */

static_assert(sizeof(gpsbb_interf_t) == 48 && sizeof(gpsbb_interf_set_t) == 208, "gpsbb_interf_t / gpsbb_interf_set_t layout");
static_assert(INTERF_MAX == GPSBB_INTERF_MAX, "INTERF_MAX");

static const uint64_t INTERF_POS_END = 1ull << 63; /* positions stay below it */

/* nearbyint(ldexp(x, 64)) for |x| <= 0.5 as a word mod 2^64 (+2^63 is -2^63 there) */
static uint64_t interf_turns(double x)
{
    double r = std::nearbyint(std::ldexp(x, 64));
    if (r >= 0x1p+63)
        r -= 0x1p+64;
    return (uint64_t)(int64_t)r;
}

extern "C" int gpsbb_interf_make(gpsbb_interf_t *e, int kind, double js_db, double f0_hz, double f1_hz, double sweep_s,
                                 double pulse_period_s, double duty, double delt)
{
    if (!e || (kind != GPSBB_INTERF_CW && kind != GPSBB_INTERF_CHIRP) || !std::isfinite(js_db) || !std::isfinite(f0_hz) ||
        !std::isfinite(delt) || !(delt > 0.0) || !std::isfinite(pulse_period_s) || pulse_period_s < 0.0)
        return GPSBB_E_BADARG;
    gpsbb_interf_t o;
    memset(&o, 0, sizeof o);
    o.kind = kind;
    const double g = std::floor(std::pow(10.0, js_db / 20.0) * 65536.0 + 0.5); /* (positive: half away from zero is half up) */
    if (!(g >= 1.0) || !(g <= 134217728.0))
        return GPSBB_E_BADARG;
    o.level_q16 = (uint32_t)g;
    const double x0 = f0_hz * delt;
    if (!(x0 >= -0.5) || !(x0 < 0.5))
        return GPSBB_E_BADARG;
    o.step = (int64_t)interf_turns(x0);
    if (kind == GPSBB_INTERF_CHIRP) {
        if (!std::isfinite(f1_hz) || !std::isfinite(sweep_s))
            return GPSBB_E_BADARG;
        const double P = std::nearbyint(sweep_s / delt), span = (f1_hz - f0_hz) * delt;
        if (!(P >= 2.0) || !(P <= 4294967295.0) || !(span >= -1.0) || !(span <= 1.0))
            return GPSBB_E_BADARG;
        o.sweep = (uint32_t)P;
        o.rate = (int64_t)interf_turns(span / P);
    }
    if (pulse_period_s > 0.0) {
        const double T = std::nearbyint(pulse_period_s / delt);
        if (!std::isfinite(duty) || !(duty > 0.0) || !(duty <= 1.0) || !(T >= 1.0) || !(T <= 4294967295.0))
            return GPSBB_E_BADARG;
        o.pulse_period = (uint32_t)T;
        const double on = std::nearbyint(duty * T);
        o.pulse_on = on < 1.0 ? 1u : (on > T ? o.pulse_period : (uint32_t)on);
    }
    *e = o;
    return GPSBB_OK;
}

/* a set the library takes, as the kernels' arguments (the launch position is interf_at's); false: GPSBB_E_BADARG */
static bool interf_args(const gpsbb_interf_set_t *set, InterfArgs *a)
{
    if (!set || set->n < 0 || set->n > GPSBB_INTERF_MAX || set->shift < 0 || set->shift > 7 || set->sample0 >= INTERF_POS_END)
        return false;
    memset(a, 0, sizeof *a);
    a->n = set->n;
    a->shift = set->shift;
    a->sample0 = set->sample0;
    for (int i = 0; i < set->n; i++) {
        const gpsbb_interf_t &e = set->e[i];
        InterfEm &o = a->e[i];
        if (e.level_q16 < 1u || e.level_q16 > (1u << 27))
            return false;
        if (e.kind == GPSBB_INTERF_CW) {
            if (e.sweep != 0u || e.rate != 0)
                return false;
        } else if (e.kind == GPSBB_INTERF_CHIRP) {
            if (e.sweep < 2u)
                return false;
        } else {
            return false;
        }
        if (e.pulse_period ? (e.pulse_on < 1u || e.pulse_on > e.pulse_period || e.pulse_offset >= e.pulse_period)
                           : (e.pulse_on != 0u || e.pulse_offset != 0u))
            return false;
        o.phase0 = e.phase0;
        o.F = (uint64_t)e.step;
        o.R = (uint64_t)e.rate;
        o.G = e.level_q16;
        o.P = e.sweep;
        if (o.P) {
            o.Phi = o.F * (uint64_t)o.P + o.R * interf_tri(o.P);
            o.magP = (uint64_t)((((unsigned __int128)1) << 64) / o.P);
        }
        if (e.pulse_period && e.pulse_on < e.pulse_period) { /* (a gate that is never off: continuous) */
            o.period = e.pulse_period;
            o.on = e.pulse_on;
            o.offset = e.pulse_offset;
            o.magG = (uint64_t)((((unsigned __int128)1) << 64) / o.period);
        }
    }
    return true;
}

/* the launch's first sample s0 and its length; false: the range reaches 2^63 */
static bool interf_at(InterfArgs *a, uint64_t s0, uint64_t nsamples)
{
    if (s0 >= INTERF_POS_END || nsamples > INTERF_POS_END - s0)
        return false;
    a->sample0 = s0;
    for (int i = 0; i < a->n; i++) {
        InterfEm &o = a->e[i];
        if (o.P) {
            o.k0 = s0 / o.P;
            o.m0 = (uint32_t)(s0 % o.P);
        }
        if (o.period)
            o.g0 = (uint32_t)((s0 + o.offset) % o.period);
    }
    return true;
}

namespace {
struct InterfHostTab {
    const int32_t *cos512, *sin512;
    void operator()(uint32_t idx, int *c, int *s) const
    {
        *c = cos512[idx];
        *s = sin512[idx];
    }
};
} // namespace

extern "C" int gpsbb_interf_eval(const gpsbb_interf_set_t *set, uint64_t s, long n, int32_t *jiq)
{
    InterfArgs a;
    if (n < 0 || (n > 0 && !jiq) || !interf_args(set, &a) || !interf_at(&a, s, (uint64_t)n))
        return GPSBB_E_BADARG;
    static int32_t sn[512], cs[512];
    static std::once_flag once;
    static bool tabs_ok = false;
    std::call_once(once, [] { tabs_ok = make_sincos(sn, cs); });
    if (!tabs_ok)
        return GPSBB_E_INTERNAL;
    const InterfHostTab tab{cs, sn};
    for (long i = 0; i < 2 * n; i++)
        jiq[i] = 0;
    /* as the kernel walks a 16-byte unit: one seek, then up to four steps */
    for (int k = 0; k < a.n; k++)
        for (long i = 0; i < n; i += 4) {
            InterfPos p = interf_seek(a.e[k], a.sample0, (uint64_t)i);
            for (long j = i; j < n && j < i + 4; j++) {
                int ji = 0, jq = 0;
                interf_step(a.e[k], p, tab, ji, jq);
                jiq[2 * j] += ji;
                jiq[2 * j + 1] += jq;
            }
        }
    return GPSBB_OK;
}

/* What happens to the render on the way out: the noise (or none) and the set (or none) of one call, checked together, at a
 * launch of nsamples from their common sample0.  Neither: the plain gather or pack. */
struct ImpairCall {
    ImpairArgs a; /* a.nz.sample0 == a.it.sample0 and a.nz.shift == a.it.shift: the launch's */
    bool noise;   /* nz was given */
    bool set;     /* a set was given (an empty one too: its shift and its range still hold) */
    bool any() const { return noise || set; }
};

/* the launch's first sample s0 and its length; false: with a set, the range reaches 2^63 */
static bool impair_at(ImpairCall *c, uint64_t s0, uint64_t nsamples)
{
    c->a.nz.sample0 = c->a.it.sample0 = s0;
    return !c->set || interf_at(&c->a.it, s0, nsamples);
}

/* nz and set as every call that takes them checks them, either or both absent; false: GPSBB_E_BADARG */
static bool impair_make(const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set, uint64_t nsamples, ImpairCall *c)
{
    memset(c, 0, sizeof *c);
    c->noise = nz != nullptr;
    c->set = set != nullptr;
    if (nz && !noise_args(nz, &c->a.nz))
        return false;
    if (set) {
        if (!interf_args(set, &c->a.it))
            return false;
        if (nz && (nz->sample0 != set->sample0 || nz->shift != set->shift))
            return false;
        c->a.nz.shift = set->shift;
    }
    return impair_at(c, set ? set->sample0 : c->a.nz.sample0, nsamples);
}

/* Enqueue what takes n int16 components at src (device memory) to dst (device memory, or host memory the device can write: pinned,
 * registered) in format fmt (0 = SC16, PACK_SC8 with shift8, PACK_SC1) on `stream`.  Returns at once.  Without impairments (ic
 * null) the plain gather or pack on GPSBB_GATHER_WGS workgroups; with them k_impair_iq on a wider grid: noise and emitters cost
 * VALU work per sample that 32 workgroups cannot issue at the rate the formats leave the GPU.  An empty set with noise
 * IS the noise launch. */
static hipError_t out_launch(gpsbb *h, int fmt, int shift8, const ImpairCall *ic, const int16_t *src, void *dst, size_t n, hipStream_t stream)
{
    if (!ic) {
        const int gwg = (int)GPSBB_KNOB_LONG("GPSBB_GATHER_WGS", 32);
        if (fmt == PACK_SC8)
            hipLaunchKernelGGL(k_pack_iq<PACK_SC8>, dim3(gwg), dim3(256), 0, stream, src, (unsigned char *)dst, n, shift8, h->d_clip.p);
        else if (fmt == PACK_SC1)
            hipLaunchKernelGGL(k_pack_iq<PACK_SC1>, dim3(gwg), dim3(256), 0, stream, src, (unsigned char *)dst, n, shift8, h->d_clip.p);
        else
            hipLaunchKernelGGL(k_gather_to_host, dim3(gwg), dim3(256), 0, stream, (const gather_u32x4 *)src, (gather_u32x4 *)dst,
                               (n * 2 + 15) / 16);
        return hipGetLastError();
    }
    ImpairArgs a = ic->a;
    a.nz.shift8 = shift8;
    const size_t nchunk = (n / 8 + PACK_UNITS - 1) / PACK_UNITS;
    const long knob = GPSBB_KNOB_LONG("GPSBB_NOISE_WGS", 256);
    const int gwg = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1L, knob), nchunk)); /* (no workgroup without work) */
    typedef void (*ImpairKernelFn)(const int16_t *, void *, size_t, ImpairArgs, const int2 *, const int32_t *, unsigned long long *,
                                   unsigned long long *);
#define GPSBB_IMPAIR_ROW(F) {k_impair_iq<F, true, false>, k_impair_iq<F, true, true>, k_impair_iq<F, false, true>}
    static const ImpairKernelFn k[3][3] = {GPSBB_IMPAIR_ROW(NOISE_SC16), GPSBB_IMPAIR_ROW(PACK_SC8), GPSBB_IMPAIR_ROW(PACK_SC1)};
#undef GPSBB_IMPAIR_ROW
    /* (a set without noise, an empty one too, runs the emitter loop: its shift still holds) */
    hipLaunchKernelGGL(k[fmt][!ic->noise ? 2 : (a.it.n > 0 ? 1 : 0)], dim3(gwg), dim3(256), 0, stream, src, dst, n, a, h->d_noise_tab.p,
                       h->d_tabs.p, h->d_nclip.p, h->d_clip.p);
    return hipGetLastError();
}

extern "C" int gpsbb_device_impair(gpsbb_t *h, const int16_t *d_src, int16_t *d_dst, long nblocks, int nsamp, const gpsbb_noise_t *nz,
                                   const gpsbb_interf_set_t *set)
{
    ImpairCall c;
    if (!h || !d_src || !d_dst || (!nz && !set) || nblocks < 1 || nsamp < 1 || (((uintptr_t)d_src | (uintptr_t)d_dst) & 1) ||
        !impair_make(nz, set, (uint64_t)nblocks * (uint64_t)nsamp, &c))
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, true); /* (noise or none: k_impair_iq is handed the table and the clip counter either way) */
    if (rc != GPSBB_OK)
        return rc;
    HIPCHK(h, out_launch(h, NOISE_SC16, 0, &c, d_src, d_dst, (size_t)nblocks * (size_t)nsamp * 2, h->s_compute));
    HIPCHK(h, hipStreamSynchronize(h->s_compute));
    return GPSBB_OK;
}

/* ---- output level (include/gpsbb.h gpsbb_level_t; gpsbb_level.hip.h) ---- */

static_assert(sizeof(gpsbb_level_t) == 536 && sizeof(LevelOut) == sizeof(gpsbb_level_t), "gpsbb_level_t layout");
static_assert(LEVEL_CLASSES == GPSBB_LEVEL_CLASSES, "LEVEL_CLASSES");

/* the header's limit: nsamp * B * B < 2^64, so that no block's sum of squares leaves 64 bits */
static bool level_fits(const ImpairArgs &a, bool noise, int nsamp)
{
    unsigned __int128 B = 32768;
    if (noise) {
        const int32_t *k = noise_knots();
        int32_t kmax = 0;
        for (int i = 0; i < NOISE_KNOTS; i++)
            kmax = std::max(kmax, k[i]);
        B += (unsigned __int128)(((long long)a.nz.s256 * kmax + (1ll << 23)) >> 24);
    }
    for (int i = 0; i < a.it.n; i++)
        B += ((unsigned long long)a.it.e[i].G * 512ull + 32768ull) >> 16;
    if (B >> 32)
        return false;
    const unsigned __int128 bb = B * B; /* < 2^64 */
    return bb * (unsigned __int128)nsamp < ((unsigned __int128)1 << 64);
}

/* How a call picks its kernel among K<noise, interf>, or for the calls that read a view K<view, noise, interf>: the table
 * [noise][interf] or [fmt][noise][interf] of every instance, indexed by what the call was given */
#define GPSBB_NI_KERNELS(K) {{K<false, false>, K<false, true>}, {K<true, false>, K<true, true>}}
#define GPSBB_VNI_ROW(K, V) {{K<V, false, false>, K<V, false, true>}, {K<V, true, false>, K<V, true, true>}}
#define GPSBB_VNI_KERNELS(K) {GPSBB_VNI_ROW(K, DS_SC16), GPSBB_VNI_ROW(K, PACK_SC8), GPSBB_VNI_ROW(K, PACK_SC1)}

/* Enqueue k_level over nblocks blocks at src into d_out (zeroed on the stream first).  The grid: the flattened (block, chunk) list,
 * at most one workgroup per CU, as k_impair_iq's. */
static hipError_t level_launch(gpsbb *h, const ImpairArgs &a, bool noise, const int16_t *src, long nblocks, int nsamp, LevelOut *d_out,
                               hipStream_t stream)
{
    const hipError_t e = hipMemsetAsync(d_out, 0, (size_t)nblocks * sizeof(LevelOut), stream);
    if (e != hipSuccess)
        return e;
    const int cpb = std::max(1, (nsamp / 4 + PACK_UNITS - 1) / PACK_UNITS);
    const long long items = (long long)nblocks * cpb;
    const int gwg = (int)std::min<long long>(256, items);
    const bool interf = a.it.n > 0;
    typedef void (*LevelKernelFn)(const int16_t *, long, int, int, ImpairArgs, const int2 *, const int32_t *, LevelOut *);
    static const LevelKernelFn k[2][2] = GPSBB_NI_KERNELS(k_level);
    hipLaunchKernelGGL(k[noise][interf], dim3(gwg), dim3(256), 0, stream, src, nblocks, nsamp, cpb, a, h->d_noise_tab.p, h->d_tabs.p, d_out);
    return hipGetLastError();
}

extern "C" int gpsbb_device_level(gpsbb_t *h, const int16_t *d_iq, long nblocks, int nsamp, const gpsbb_noise_t *nz,
                                  const gpsbb_interf_set_t *set, gpsbb_level_t *out)
{
    ImpairCall c;
    if (!h || !d_iq || !out || nblocks < 1 || nsamp < 1 || ((uintptr_t)d_iq & 3) ||
        !impair_make(nz, set, (uint64_t)nblocks * (uint64_t)nsamp, &c) || !level_fits(c.a, c.noise, nsamp))
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, c.noise);
    if (rc != GPSBB_OK)
        return rc;
    HIPCHK(h, (hipError_t)h->d_level.reserve((size_t)nblocks));
    HIPCHK(h, level_launch(h, c.a, c.noise, d_iq, nblocks, nsamp, h->d_level.p, h->s_compute));
    HIPCHK(h, hipMemcpyAsync(out, h->d_level.p, (size_t)nblocks * sizeof(LevelOut), hipMemcpyDeviceToHost, h->s_compute));
    HIPCHK(h, hipStreamSynchronize(h->s_compute));
    return GPSBB_OK;
}

/* components of lv[0 .. n) with m(x) > k, per component summed */
static uint64_t level_above(const gpsbb_level_t *lv, long n, int k)
{
    uint64_t t = 0;
    for (long b = 0; b < n; b++)
        for (int c = 0; c < 2; c++)
            for (int m = k + 1; m < GPSBB_LEVEL_CLASSES; m++)
                t += lv[b].hist[c][m];
    return t;
}

/* the two identities of the header: (clip16, clip8) at (a, shift8); sc8: the format is SC8 */
static void level_clips(const gpsbb_level_t *lv, long n, int a, bool sc8, int shift8, uint64_t *clip16, uint64_t *clip8)
{
    const uint64_t sat = level_above(lv, n, 15 + a);
    *clip16 = sat;
    *clip8 = 0;
    if (sc8) {
        const int top = std::min(7 + shift8 + a, 15 + a); /* classes (top, 15 + a] clamp in SC8 without having saturated */
        *clip8 = level_above(lv, n, top) - sat + (shift8 < 8 ? sat : 0);
    }
}

/* the format bits of fmt: 0 SC16, 1 SC8, 2 SC1; -1 unknown */
static int level_format(unsigned fmt)
{
    const unsigned f = (fmt & GPSBB_OUT_FORMAT_MASK) >> 8;
    return f > 2 ? -1 : (int)f;
}

extern "C" int gpsbb_level_clips(const gpsbb_level_t *lv, long n, int shift, unsigned fmt, uint64_t *clip16, uint64_t *clip8)
{
    const unsigned sh8 = (fmt & GPSBB_OUT_SHIFT_MASK) >> 12;
    const int f = level_format(fmt);
    if (!lv || n < 1 || shift < 0 || shift > 7 || f < 0 || (fmt >> 16) || (fmt & 0xffu) || (sh8 && f != 1))
        return GPSBB_E_BADARG;
    uint64_t c16, c8;
    level_clips(lv, n, shift, f == 1, (int)sh8, &c16, &c8);
    if (clip16) *clip16 = c16;
    if (clip8) *clip8 = c8;
    return GPSBB_OK;
}

extern "C" int gpsbb_level_choose(const gpsbb_level_t *lv, long n, unsigned fmt, double clip_ppm, int *shift, int *shift8)
{
    const int f = level_format(fmt);
    if (!lv || n < 1 || f < 0 || !(clip_ppm >= 0.0) || !shift || !shift8)
        return GPSBB_E_BADARG;
    uint64_t total = 0;
    for (long b = 0; b < n; b++)
        total += lv[b].n;
    const double bd = std::floor(clip_ppm * 1e-6 * (double)(2 * total));
    const uint64_t budget = bd >= 0x1p+64 ? ~0ull : (uint64_t)bd;
    int over = 0, a = 0, q = 0;
    uint64_t c16 = 0, c8 = 0;
    for (a = 0; a <= 7; a++) {
        level_clips(lv, n, a, false, 0, &c16, &c8);
        if (c16 <= budget)
            break;
    }
    if (a > 7) {
        a = 7;
        over = 1;
    }
    if (f == 1 && over) {
        q = 15; /* nothing scales this into int16: both largest values */
    } else if (f == 1) {
        for (q = 0; q <= 15; q++) {
            level_clips(lv, n, a, true, q, &c16, &c8);
            if (c8 <= budget)
                break;
        }
        if (q > 15) {
            q = 15;
            over = 1;
        }
    }
    *shift = a;
    *shift8 = q;
    return over;
}

extern "C" double gpsbb_level_rms(const gpsbb_level_t *lv, long n, int component)
{
    if (!lv || n < 1 || component < 0 || component > 1)
        return NAN;
    long double sq = 0.0L, cnt = 0.0L;
    for (long b = 0; b < n; b++) {
        sq += (long double)lv[b].sumsq[component];
        cnt += (long double)lv[b].n;
    }
    return cnt > 0.0L ? (double)sqrtl(sq / cnt) : NAN;
}

/* ---- despreading: the render read back the way its consumer reads it (include/gpsbb.h, gpsbb_despread.hip.h) ---- */

extern "C" long gpsbb_despread_segments(long nsamp, int seg_tiles)
{
    if (nsamp < 1 || seg_tiles < 1)
        return GPSBB_E_BADARG;
    const long len = (long)TILE * seg_tiles;
    return (nsamp + len - 1) / len;
}

/* the kernel of a despreading call: K<view, noise, g, interf> for every view, with and without noise, for every state granule
 * (BatchDev::st_log2), without and with the set's J in the view (gpsbb_batch_despread_impaired) */
#define GPSBB_DS_G(K, V, N, J) {K<V, N, 0, J>, K<V, N, 1, J>, K<V, N, 2, J>}
#define GPSBB_DS_V(K, V, J) {GPSBB_DS_G(K, V, false, J), GPSBB_DS_G(K, V, true, J)}
#define GPSBB_DS_KERNEL(FN, NAME, K)                                                                                                    \
    static FN NAME(int view, bool noise, int g, bool interf)                                                                            \
    {                                                                                                                                   \
        static const FN k[2][3][2][EV_STATE_LOG2_MAX + 1] = {{GPSBB_DS_V(K, DS_SC16, false), GPSBB_DS_V(K, PACK_SC8, false), GPSBB_DS_V(K, PACK_SC1, false)}, \
                                                             {GPSBB_DS_V(K, DS_SC16, true), GPSBB_DS_V(K, PACK_SC8, true), GPSBB_DS_V(K, PACK_SC1, true)}};    \
        return k[interf ? 1 : 0][view][noise ? 1 : 0][g];                                                                               \
    }
typedef void (*DsKernelFn)(BatchDev, DsArgs);
typedef void (*DslKernelFn)(BatchDev, DslArgs);
GPSBB_DS_KERNEL(DsKernelFn, ds_kernel, k_despread)
GPSBB_DS_KERNEL(DslKernelFn, dsl_kernel, k_despread_lags) /* ... at lags (gpsbb_batch_despread_lags) */
#undef GPSBB_DS_KERNEL
#undef GPSBB_DS_V
#undef GPSBB_DS_G

/* The view of a call that reads device IQ (gpsbb_batch_despread*, gpsbb_device_acquire, _track, _fir): the samples, PACK_SC8's
 * shift and the call's impairments, everything else zero.  After iq_call_begin, which makes the table. */
static DsArgs iq_view(const gpsbb *h, const void *d_iq, int shift8, const ImpairCall &ic)
{
    DsArgs d;
    memset(&d, 0, sizeof d);
    d.iq = static_cast<const uint32_t *>(d_iq);
    d.shift8 = shift8;
    d.nz = ic.a.nz;
    d.ntab = h->d_noise_tab.p;
    d.it = ic.a.it;
    return d;
}

/* the argument checks of every despreading call, in the order the tests pin, and what they settle of its arguments: the lags, the
 * source and the view's shift (al->d.iq, al->d.shift8).  *fmt: the view's kernel number; *ic: the impairments, for iq_view */
static int ds_make_args(gpsbb_batch_t *b, const int16_t *d_iq, unsigned view, const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set,
                        int seg_tiles, const int *lags, int nlags, const gpsbb_corr_t *out, DslArgs *al, int *fmt, ImpairCall *ic)
{
    if (!b)
        return GPSBB_E_BADARG;
    const BatchPlan &pl = b->plan;
    memset(al, 0, sizeof *al);
    if (!impair_make(nz, set, (uint64_t)pl.nblocks * (uint64_t)pl.nsamp, ic))
        return GPSBB_E_BADARG;
    /* (nothing is packed here, so SC1 takes any nsamp: the format is looked up for a length it accepts) */
    *fmt = (view & ~(GPSBB_OUT_FORMAT_MASK | GPSBB_OUT_SHIFT_MASK)) ? -1 : out_format(view, 4, &al->d.shift8);
    if (!out || seg_tiles < 1 || *fmt < 0 || ((uintptr_t)d_iq & 3))
        return GPSBB_E_BADARG;
    for (int l = 0; lags && l < nlags; l++) {
        al->lags[l] = lags[l];
        al->halo_lo |= lags[l] < 0;
        al->halo_hi |= lags[l] > 0;
    }
    al->nlags = nlags;
    if (!b->ran)
        return GPSBB_E_STATE;
    /* the two limits of this call: the accumulator's batches, and runs of the per-sample kernel, which leave rows and no
     * tile states */
    if ((pl.flags & GPSBB_FIXED_CARRIER) || !pl.ev)
        return GPSBB_E_BADARG;
    al->d.iq = reinterpret_cast<const uint32_t *>(d_iq ? d_iq : b->last_iq);
    return al->d.iq ? GPSBB_OK : GPSBB_E_STATE; /* the last run rendered into the caller's buffer: it has to be named */
}

/* pure: the tiles a wavefront takes at a time and the workgroups of a block, for a device of cus compute units.  A chunk never
 * spans more segments than it must, and small batches hand their tiles out one at a time */
static void ds_geometry(int nblocks, int ntiles, int seg_tiles, long cus, int &chunk, int &wgs_per_block)
{
    chunk = seg_tiles < DS_CHUNK ? seg_tiles : DS_CHUNK;
    while (chunk > 1 && (long)nblocks * (((long)ntiles + chunk - 1) / chunk) < cus * 8 * DS_WAVES)
        chunk--;
    const long chunks = ((long)ntiles + chunk - 1) / chunk, max_useful = (chunks + DS_WAVES - 1) / DS_WAVES;
    const long want = (cus * 16 + nblocks - 1) / nblocks;
    wgs_per_block = (int)(want < 1 ? 1 : (want > max_useful ? max_useful : want));
}

/* every despreading call: the checks, then scratch, geometry, launch and copy-back.  lags == nullptr: the prompt sums by k_despread,
 * out [nblocks][nch][nseg]; otherwise k_despread_lags at lags[0 .. nlags), out [nblocks][nch][nseg][nlags] */
static int batch_despread(gpsbb_batch_t *b, const int16_t *d_iq, unsigned view, const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set,
                          int seg_tiles, const int *lags, int nlags, gpsbb_corr_t *out)
{
    DslArgs al;
    ImpairCall ic;
    int fmt = -1, rc = ds_make_args(b, d_iq, view, nz, set, seg_tiles, lags, nlags, out, &al, &fmt, &ic);
    if (rc != GPSBB_OK)
        return rc;
    gpsbb *h = b->h;
    const BatchPlan &pl = b->plan;
    DsArgs &a = al.d;
    rc = iq_call_begin(h, ic.noise);
    if (rc != GPSBB_OK)
        return rc;
    a = iq_view(h, a.iq, a.shift8, ic);
    a.seg_tiles = seg_tiles;
    a.nseg = (int)gpsbb_despread_segments(pl.nsamp, seg_tiles);
    a.danger = (uint32_t)GPSBB_KNOB_LONG("GPSBB_DS_DANGER", 2u * PD_BAND); /* (larger: more samples take the exact path; a test aid) */
    /* ---- scratch, zeroed: the sums, behind them the count of exact-path samples; the blocks' tile counters ---- */
    const size_t nsum = (size_t)pl.nblocks * pl.nch * (size_t)a.nseg * (size_t)(lags ? nlags : 1) * 2;
    HIPCHK(h, (hipError_t)b->d_ds.reserve(nsum + 1));
    HIPCHK(h, (hipError_t)b->d_ds_ctr.reserve((size_t)pl.nblocks));
    hipStream_t cs = h->s_compute;
    HIPCHK(h, hipMemsetAsync(b->d_ds.p, 0, (nsum + 1) * sizeof(unsigned long long), cs));
    HIPCHK(h, hipMemsetAsync(b->d_ds_ctr.p, 0, (size_t)pl.nblocks * sizeof(int32_t), cs));
    a.out = b->d_ds.p;
    a.n_exact = b->d_ds.p + nsum;
    a.ctr = b->d_ds_ctr.p;
    /* ---- launch ---- */
    ds_geometry(pl.nblocks, pl.ntiles, seg_tiles, cu_count(h->sm_count), a.chunk, a.wgs_per_block);
    const BatchDev p = batch_dev(b, b->sets[b->last_set], batch_launch_plan(b));
    HIPCHK(h, b->ds_tm.start(cs));
    const dim3 grid((unsigned)((long)a.wgs_per_block * pl.nblocks));
    if (lags)
        hipLaunchKernelGGL(dsl_kernel(fmt, ic.noise, p.st_log2, ic.set), grid, dim3(DS_WG), 0, cs, p, al);
    else
        hipLaunchKernelGGL(ds_kernel(fmt, ic.noise, p.st_log2, ic.set), grid, dim3(DS_WG), 0, cs, p, a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, b->ds_tm.stop(cs));
    /* ---- copy back ---- */
    HIPCHK(h, hipMemcpyAsync(out, b->d_ds.p, nsum * sizeof(unsigned long long), hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipMemcpyAsync(&b->ds_last_exact, b->d_ds.p + nsum, sizeof(unsigned long long), hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipStreamSynchronize(cs));
    return GPSBB_OK;
}

extern "C" int gpsbb_batch_despread(gpsbb_batch_t *b, const int16_t *d_iq, unsigned view, const gpsbb_noise_t *nz, int seg_tiles,
                                    gpsbb_corr_t *out)
{
    return batch_despread(b, d_iq, view, nz, nullptr, seg_tiles, nullptr, 0, out);
}

extern "C" int gpsbb_batch_despread_impaired(gpsbb_batch_t *b, const int16_t *d_iq, unsigned view, const gpsbb_noise_t *nz,
                                             const gpsbb_interf_set_t *set, int seg_tiles, gpsbb_corr_t *out)
{
    return batch_despread(b, d_iq, view, nz, set, seg_tiles, nullptr, 0, out);
}

extern "C" int gpsbb_batch_despread_lags(gpsbb_batch_t *b, const int16_t *d_iq, unsigned view, const gpsbb_noise_t *nz,
                                         const gpsbb_interf_set_t *set, int seg_tiles, const int *lags, int nlags, gpsbb_corr_t *out)
{
    if (!lags || nlags < 1 || nlags > GPSBB_DESPREAD_MAX_LAGS)
        return GPSBB_E_BADARG;
    for (int l = 0; l < nlags; l++)
        if (lags[l] < -GPSBB_DESPREAD_MAX_LAG || lags[l] > GPSBB_DESPREAD_MAX_LAG)
            return GPSBB_E_BADARG;
    return batch_despread(b, d_iq, view, nz, set, seg_tiles, lags, nlags, out);
}

/* ---- blind acquisition (include/gpsbb.h gpsbb_device_acquire; gpsbb_acq.h, gpsbb_acq.hip.h) ---- */

static_assert(sizeof(gpsbb_acq_cfg_t) == 288 && sizeof(gpsbb_acq_row_t) == 32, "gpsbb_acq_cfg_t / gpsbb_acq_row_t layout");

extern "C" int gpsbb_acq_min_shift(unsigned view, int ncoh, int nnc) { return acq_min_shift(view, ncoh, nnc); }

extern "C" int gpsbb_acq_make(gpsbb_acq_cfg_t *cfg, double delt, double f_min_hz, double f_step_hz, int nbins, double coh_s, int nlags,
                              int nnc, unsigned view)
{
    return acq_make(cfg, delt, f_min_hz, f_step_hz, nbins, coh_s, nlags, nnc, view);
}

extern "C" int gpsbb_acq_best(const gpsbb_acq_row_t *rows, const gpsbb_acq_cfg_t *cfg, int prn, int *bin, int *lag, uint64_t *peak,
                              double *ratio)
{
    return acq_best(rows, cfg, prn, bin, lag, peak, ratio);
}

typedef void (*AcqKernelFn)(AcqArgs);
static AcqKernelFn acq_kernel(int fmt, bool noise, bool interf)
{
    static const AcqKernelFn k[3][2][2] = GPSBB_VNI_KERNELS(k_acq);
    return k[fmt][noise][interf];
}

extern "C" int gpsbb_device_acquire(gpsbb_t *h, const int16_t *d_iq, long nsamp, unsigned view, const gpsbb_noise_t *nz,
                                    const gpsbb_interf_set_t *set, const gpsbb_acq_cfg_t *cfg, gpsbb_acq_row_t *rows, uint64_t *grid)
{
    int shift8 = 0;
    const int fmt = acq_view_format(view, &shift8);
    ImpairCall ic;
    if (!h || !d_iq || !cfg || !rows || ((uintptr_t)d_iq & 3) || nsamp < 1 || !acq_cfg_ok(cfg, fmt, nsamp) ||
        !impair_make(nz, set, (uint64_t)nsamp, &ic))
        return GPSBB_E_BADARG;
    static_assert(DS_SC16 == 0 && PACK_SC8 == 1 && PACK_SC1 == 2, "acq_view_format's numbers are the kernels'");
    const int rc = iq_call_begin(h, ic.noise);
    if (rc != GPSBB_OK)
        return rc;
    AcqArgs a;
    memset(&a, 0, sizeof a);
    a.nbins = cfg->nbins;
    a.ncoh = cfg->ncoh;
    a.npad = (cfg->ncoh + 31) & ~31;
    a.nlags = cfg->nlags;
    a.nnc = cfg->nnc;
    a.shift = cfg->shift;
    a.ntiles = (cfg->nlags + 31) / 32;
    a.nsamp = nsamp;
    memcpy(a.step, cfg->step, sizeof a.step);
    const size_t nrows = (size_t)ACQ_PRNS * (size_t)a.nbins;
    const size_t chip_words = ((size_t)a.nnc * ACQ_PRNS * (size_t)a.npad + 7) / 8;
    const size_t row_words = nrows * ((size_t)a.ntiles + 1) * (sizeof(gpsbb_acq_row_t) / 8);
    const size_t grid_words = grid ? nrows * (size_t)a.nlags : 0;
    HIPCHK(h, (hipError_t)h->d_acq_chips.reserve(chip_words));
    HIPCHK(h, (hipError_t)h->d_acq_rows.reserve(row_words));
    if (grid)
        HIPCHK(h, (hipError_t)h->d_acq_grid.reserve(grid_words));
    hipStream_t cs = h->s_compute;
    gpsbb_acq_row_t *d_part = reinterpret_cast<gpsbb_acq_row_t *>(h->d_acq_rows.p);
    gpsbb_acq_row_t *d_rows = d_part + nrows * (size_t)a.ntiles;
    HIPCHK(h, hipMemsetAsync(h->d_acq_rows.p, 0, row_words * 8, cs));
    if (grid)
        HIPCHK(h, hipMemsetAsync(h->d_acq_grid.p, 0, grid_words * 8, cs));
    a.d = iq_view(h, d_iq, shift8, ic);
    a.tabs = h->d_tabs.p;
    a.chips = reinterpret_cast<const int8_t *>(h->d_acq_chips.p);
    a.grid = grid ? h->d_acq_grid.p : nullptr;
    a.part = d_part;
    const long long nchip = (long long)a.nnc * a.npad;
    HIPCHK(h, h->acq_tm.start(cs));
    hipLaunchKernelGGL(k_acq_chips, dim3((unsigned)((nchip + 255) / 256)), dim3(256), 0, cs, h->d_ca.p, reinterpret_cast<int8_t *>(h->d_acq_chips.p),
                       cfg->prn_mask, (unsigned long long)cfg->code_step, a.ncoh, a.npad, a.nnc);
    HIPCHK(h, hipGetLastError());
    /* x: runs of four delay tiles (at most 256), y: the bins (at most 64) */
    hipLaunchKernelGGL(acq_kernel(fmt, ic.noise, ic.set), dim3((unsigned)((a.ntiles + AQ_WAVES - 1) / AQ_WAVES), (unsigned)a.nbins),
                       dim3(AQ_WG), 0, cs, a);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_acq_fold, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, cs, d_part, d_rows, (int)nrows, a.ntiles);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->acq_tm.stop(cs));
    HIPCHK(h, hipMemcpyAsync(rows, d_rows, nrows * sizeof(gpsbb_acq_row_t), hipMemcpyDeviceToHost, cs));
    if (grid)
        HIPCHK(h, hipMemcpyAsync(grid, h->d_acq_grid.p, grid_words * 8, hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipStreamSynchronize(cs));
    h->d_acq_grid.release(); /* the grid is not kept: it can be half a gigabyte, and the next call may not want one */
    return GPSBB_OK;
}

/* ---- blind tracking (include/gpsbb.h gpsbb_device_track; gpsbb_track.h, gpsbb_track.hip.h) ---- */

static_assert(sizeof(gpsbb_trk_cfg_t) == 48 && sizeof(gpsbb_trk_state_t) == 80 && sizeof(gpsbb_trk_epoch_t) == 96,
              "gpsbb_trk_cfg_t / gpsbb_trk_state_t / gpsbb_trk_epoch_t layout");

extern "C" int gpsbb_trk_make(gpsbb_trk_cfg_t *cfg, double delt, double fll_gain, double pll_bw_hz, double dll_gain, int nfll, int max_epochs)
{
    return trk_make(cfg, delt, fll_gain, pll_bw_hz, dll_gain, nfll, max_epochs);
}

extern "C" int gpsbb_trk_seed(gpsbb_trk_state_t *state, const gpsbb_acq_cfg_t *acq_cfg, int prn, int bin, int lag)
{
    return trk_seed(state, acq_cfg, prn, bin, lag);
}

extern "C" int gpsbb_trk_bitsync(const gpsbb_trk_epoch_t *epochs, int n, int skip, int *offset, int32_t hist[20])
{
    return trk_bitsync(epochs, n, skip, offset, hist);
}

extern "C" int gpsbb_trk_bits(const gpsbb_trk_epoch_t *epochs, int n, int first, int8_t *bits, int max)
{
    return trk_bits(epochs, n, first, bits, max);
}

typedef void (*TrkKernelFn)(TrkArgs);
static TrkKernelFn trk_kernel(int fmt, bool noise, bool interf)
{
    static const TrkKernelFn k[3][2][2] = GPSBB_VNI_KERNELS(k_track);
    return k[fmt][noise][interf];
}

extern "C" int gpsbb_device_track(gpsbb_t *h, const int16_t *d_iq, long nsamp, unsigned view, const gpsbb_noise_t *nz,
                                  const gpsbb_interf_set_t *set, const gpsbb_trk_cfg_t *cfg, gpsbb_trk_state_t *states, int nch,
                                  gpsbb_trk_epoch_t *epochs, int32_t *counts)
{
    int shift8 = 0;
    const int fmt = acq_view_format(view, &shift8);
    ImpairCall ic;
    if (!h || !d_iq || !cfg || !states || !epochs || !counts || ((uintptr_t)d_iq & 3) || nsamp < 1 || nch < 1 || nch > TRK_MAX_CH || fmt < 0 ||
        !trk_cfg_ok(cfg) || !impair_make(nz, set, (uint64_t)nsamp, &ic))
        return GPSBB_E_BADARG;
    for (int c = 0; c < nch; c++)
        if (!trk_state_ok(&states[c], nsamp))
            return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, ic.noise);
    if (rc != GPSBB_OK)
        return rc;
    /* ---- scratch, in 8-byte words: the states, the counts, the records ---- */
    const size_t st_words = (size_t)nch * sizeof(gpsbb_trk_state_t) / 8, cnt_words = ((size_t)nch + 1) / 2;
    const size_t rec_words = (size_t)nch * (size_t)cfg->max_epochs * (sizeof(gpsbb_trk_epoch_t) / 8);
    HIPCHK(h, (hipError_t)h->d_trk.reserve(st_words + cnt_words + rec_words));
    hipStream_t cs = h->s_compute;
    TrkArgs a;
    memset(&a, 0, sizeof a);
    a.d = iq_view(h, d_iq, shift8, ic);
    a.tabs = h->d_tabs.p;
    a.ca_bits = h->d_ca.p;
    a.cfg = *cfg;
    a.states = reinterpret_cast<gpsbb_trk_state_t *>(h->d_trk.p);
    a.counts = reinterpret_cast<int32_t *>(h->d_trk.p + st_words);
    a.epochs = reinterpret_cast<gpsbb_trk_epoch_t *>(h->d_trk.p + st_words + cnt_words);
    a.nsamp = nsamp;
    HIPCHK(h, hipMemcpyAsync(a.states, states, (size_t)nch * sizeof(gpsbb_trk_state_t), hipMemcpyHostToDevice, cs));
    HIPCHK(h, hipMemsetAsync(a.counts, 0, cnt_words * 8, cs));
    HIPCHK(h, h->trk_tm.start(cs));
    hipLaunchKernelGGL(trk_kernel(fmt, ic.noise, ic.set), dim3((unsigned)nch), dim3(TK_WG), 0, cs, a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->trk_tm.stop(cs));
    /* ---- copy back: the counts first, then each channel's records as far as they go, and the states ---- */
    int32_t n_out[TRK_MAX_CH];
    gpsbb_trk_state_t st_out[TRK_MAX_CH];
    HIPCHK(h, hipMemcpyAsync(n_out, a.counts, (size_t)nch * sizeof(int32_t), hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipMemcpyAsync(st_out, a.states, (size_t)nch * sizeof(gpsbb_trk_state_t), hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipStreamSynchronize(cs));
    for (int c = 0; c < nch; c++) {
        if (n_out[c] < 0 || n_out[c] > cfg->max_epochs)
            return GPSBB_E_INTERNAL;
        if (n_out[c])
            HIPCHK(h, hipMemcpyAsync(epochs + (size_t)c * (size_t)cfg->max_epochs, a.epochs + (size_t)c * (size_t)cfg->max_epochs,
                                     (size_t)n_out[c] * sizeof(gpsbb_trk_epoch_t), hipMemcpyDeviceToHost, cs));
    }
    HIPCHK(h, hipStreamSynchronize(cs));
    memcpy(states, st_out, (size_t)nch * sizeof(gpsbb_trk_state_t));
    memcpy(counts, n_out, (size_t)nch * sizeof(int32_t));
    return GPSBB_OK;
}

/* ---- the front-end filter (include/gpsbb.h gpsbb_device_fir; gpsbb_fir.h, gpsbb_fir.hip.h) ---- */

static_assert(sizeof(gpsbb_fir_t) == 276, "gpsbb_fir_t layout");

extern "C" int gpsbb_fir_make(gpsbb_fir_t *f, int ntaps, int decim, double cutoff, double atten_db)
{
    return fir_make(f, ntaps, decim, cutoff, atten_db);
}

typedef void (*FirKernelFn)(FirArgs);
static FirKernelFn fir_kernel(bool noise, bool interf)
{
    static const FirKernelFn k[2][2] = GPSBB_NI_KERNELS(k_fir);
    return k[noise][interf];
}

extern "C" int gpsbb_device_fir(gpsbb_t *h, const int16_t *d_iq, long nsamp, const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set,
                                const gpsbb_fir_t *fir, const int16_t *hist_in, int16_t *hist_out, int16_t *d_out, uint64_t *clipped)
{
    ImpairCall ic;
    if (!h || !d_iq || !fir || !d_out || (((uintptr_t)d_iq | (uintptr_t)d_out) & 3) || nsamp < 1 || !fir_ok(fir) || nsamp % fir->decim ||
        !impair_make(nz, set, (uint64_t)nsamp, &ic))
        return GPSBB_E_BADARG;
    const int T = fir->ntaps, D = fir->decim, Te = T + (T & 1);
    const long nout = nsamp / D, tiles = (nout + FIR_TILE - 1) / FIR_TILE;
    const uintptr_t in0 = (uintptr_t)d_iq, in1 = in0 + 4 * (uintptr_t)nsamp, out0 = (uintptr_t)d_out, out1 = out0 + 4 * (uintptr_t)nout;
    if ((out0 < in1 && in0 < out1) || tiles > 0x7fffffffL)
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, ic.noise);
    if (rc != GPSBB_OK)
        return rc;
    /* ---- scratch, in 8-byte words: the clip count, then room for the longest history twice ---- */
    constexpr size_t hist_words = (GPSBB_FIR_MAX_TAPS - 1) / 2;
    HIPCHK(h, (hipError_t)h->d_fir.reserve(1 + 2 * hist_words));
    hipStream_t cs = h->s_compute;
    FirArgs a;
    memset(&a, 0, sizeof a);
    a.d = iq_view(h, d_iq, 0, ic);
    a.tabs = h->d_tabs.p;
    a.clipped = h->d_fir.p;
    uint32_t *d_hist_in = reinterpret_cast<uint32_t *>(h->d_fir.p + 1), *d_hist_out = reinterpret_cast<uint32_t *>(h->d_fir.p + 1 + hist_words);
    a.hist_in = d_hist_in;
    a.hist_out = d_hist_out;
    a.out = reinterpret_cast<uint32_t *>(d_out);
    a.nsamp = nsamp;
    a.nout = nout;
    a.T = T;
    a.Te = Te;
    a.D = D;
    a.shift = fir->shift;
    a.PL = fir_plane(Te, D);
    a.npairs = Te / 2;
    a.rcp = ((1u << FIR_RCP_BITS) + (uint32_t)D - 1u) / (uint32_t)D;
    for (int j = 0; j < a.npairs; j++) {
        const int k = 2 * j, c = Te - 2 - k;
        a.hp[j] = ((uint32_t)(uint16_t)(k + 1 < T ? fir->h[k + 1] : 0)) | ((uint32_t)(uint16_t)fir->h[k] << 16);
        a.off[j] = (uint32_t)((c % D) * a.PL + c / D);
    }
    HIPCHK(h, hipMemsetAsync(h->d_fir.p, 0, (1 + 2 * hist_words) * 8, cs));
    if (hist_in && T > 1)
        HIPCHK(h, hipMemcpyAsync(d_hist_in, hist_in, (size_t)(T - 1) * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(h, h->fir_tm.start(cs));
    hipLaunchKernelGGL(fir_kernel(ic.noise, ic.set), dim3((unsigned)tiles), dim3(FIR_WG), fir_lds_bytes(Te, D), cs, a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->fir_tm.stop(cs));
    uint32_t tail[GPSBB_FIR_MAX_TAPS];
    unsigned long long clips = 0;
    HIPCHK(h, hipMemcpyAsync(&clips, a.clipped, sizeof clips, hipMemcpyDeviceToHost, cs));
    if (T > 1)
        HIPCHK(h, hipMemcpyAsync(tail, d_hist_out, (size_t)(T - 1) * 4, hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipStreamSynchronize(cs));
    if (hist_out && T > 1)
        memcpy(hist_out, tail, (size_t)(T - 1) * 4);
    if (clipped)
        *clipped = clips;
    return GPSBB_OK;
}

/* ---- the power spectrum (include/gpsbb.h gpsbb_device_psd; gpsbb_psd.h, gpsbb_psd.hip.h) ---- */

static_assert(sizeof(gpsbb_psd_t) == 8208 && sizeof(psd_c) == 8, "gpsbb_psd_t layout");

/* the table, made once: c [2048] then s [2048] */
static const int32_t *psd_table()
{
    static const std::vector<int32_t> t = [] {
        std::vector<int32_t> v(2 * PSD_TW);
        psd_twiddles(v.data(), v.data() + PSD_TW);
        return v;
    }();
    return t.data();
}

extern "C" int gpsbb_psd_twiddles(int32_t c[2048], int32_t s[2048])
{
    if (!c || !s)
        return GPSBB_E_BADARG;
    memcpy(c, psd_table(), PSD_TW * sizeof(int32_t));
    memcpy(s, psd_table() + PSD_TW, PSD_TW * sizeof(int32_t));
    return GPSBB_OK;
}

extern "C" int gpsbb_psd_min_shift(long nseg) { return psd_min_shift(nseg); }

extern "C" int gpsbb_psd_make(gpsbb_psd_t *p, int log2n, long hop, int window, long nsamp) { return psd_make(p, log2n, hop, window, nsamp); }

extern "C" double gpsbb_psd_scale(const gpsbb_psd_t *p, long nseg, unsigned view)
{
    int shift8 = 0;
    return psd_scale(p, nseg, acq_view_format(view, &shift8));
}

/* d_psd_tab, in 8-byte words: k_psd's table (uploaded when the buffer is made), then room for a window and a result */
constexpr size_t win_words = GPSBB_PSD_MAX_N / 4;
static hipError_t psd_tab_ready(gpsbb *h)
{
    if (h->d_psd_tab.p)
        return hipSuccess;
    hipError_t e = (hipError_t)h->d_psd_tab.reserve(PSD_TW + win_words + GPSBB_PSD_MAX_N);
    if (e != hipSuccess)
        return e;
    std::vector<psd_c> tw(PSD_TW); /* k_psd's order: entry brev11(2 y) at y, y < 1024 (the second half is not read) */
    for (uint32_t y = 0; y < (uint32_t)PSD_TW; y++)
        tw[y] = psd_c{psd_table()[psd_brev11(2 * y & 2047u)], psd_table()[PSD_TW + psd_brev11(2 * y & 2047u)]};
    e = hipMemcpy(h->d_psd_tab.p, tw.data(), PSD_TW * sizeof(psd_c), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        release_all(h->d_psd_tab); /* the table or no buffer: the next call uploads again */
    return e;
}

typedef void (*PsdKernelFn)(PsdArgs);
static PsdKernelFn psd_kernel(int fmt, bool noise, bool interf)
{
    static const PsdKernelFn k[3][2][2] = GPSBB_VNI_KERNELS(k_psd);
    return k[fmt][noise][interf];
}

extern "C" int gpsbb_device_psd(gpsbb_t *h, const int16_t *d_iq, long nsamp, unsigned view, const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set,
                                const gpsbb_psd_t *p, uint64_t *psd, long *nseg_out)
{
    int shift8 = 0;
    const int fmt = acq_view_format(view, &shift8);
    ImpairCall ic;
    long nseg = 0;
    if (!h || !d_iq || !p || !psd || ((uintptr_t)d_iq & 3) || fmt < 0 || !psd_ok(p, nsamp, &nseg) || !impair_make(nz, set, (uint64_t)nsamp, &ic))
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, ic.noise);
    if (rc != GPSBB_OK)
        return rc;
    const int L = p->log2n, N = 1 << L;
    int run = 0, nwg = 0;
    psd_geometry(L, nseg, &run, &nwg);
    /* ---- scratch, in 8-byte words: the table (uploaded when the buffer is made), the window, the result; the partials ---- */
    hipStream_t cs = h->s_compute;
    HIPCHK(h, psd_tab_ready(h));
    HIPCHK(h, (hipError_t)h->d_psd.reserve((size_t)nwg * (size_t)N));
    PsdArgs a;
    memset(&a, 0, sizeof a);
    a.d = iq_view(h, d_iq, shift8, ic);
    a.tabs = h->d_tabs.p;
    a.tw = reinterpret_cast<const psd_c *>(h->d_psd_tab.p);
    int16_t *d_win = reinterpret_cast<int16_t *>(h->d_psd_tab.p + PSD_TW);
    unsigned long long *d_out = h->d_psd_tab.p + PSD_TW + win_words;
    a.win = d_win;
    a.part = h->d_psd.p;
    a.nseg = nseg;
    a.hop = p->hop;
    a.run = run;
    a.log2n = L;
    a.shift = p->shift;
    a.wmul = 1 << (15 - psd_wbits(fmt));
    HIPCHK(h, hipMemcpyAsync(d_win, p->win, (size_t)N * sizeof(int16_t), hipMemcpyHostToDevice, cs));
    HIPCHK(h, h->psd_tm.start(cs));
    hipLaunchKernelGGL(psd_kernel(fmt, ic.noise, ic.set), dim3((unsigned)nwg), dim3(PSD_WG), psd_lds_bytes(L), cs, a);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_psd_fold, dim3((unsigned)(N / PSD_FOLD_BINS)), dim3(PSD_FOLD_BINS * PSD_FOLD_SLICES), 0, cs, h->d_psd.p, d_out, L, nwg);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->psd_tm.stop(cs));
    std::vector<uint64_t> out((size_t)N);
    HIPCHK(h, hipMemcpyAsync(out.data(), d_out, (size_t)N * sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipStreamSynchronize(cs));
    memcpy(psd, out.data(), (size_t)N * sizeof(uint64_t));
    if (nseg_out)
        *nseg_out = nseg;
    return GPSBB_OK;
}

/* ---- interference excision (include/gpsbb.h gpsbb_device_excise; gpsbb_exc.h, gpsbb_exc.hip.h) ---- */

static_assert(sizeof(gpsbb_exc_t) == 8720 && sizeof(exc_tw) == 16, "gpsbb_exc_t layout");

extern "C" int gpsbb_exc_make(gpsbb_exc_t *e, int log2n) { return exc_make(e, log2n); }

extern "C" int gpsbb_exc_from_psd(gpsbb_exc_t *e, const uint64_t *psd, const gpsbb_psd_t *p, long nseg, double mask_db, double thr_db)
{
    return exc_from_psd(e, psd, p, nseg, mask_db, thr_db);
}

typedef void (*ExcKernelFn)(ExcArgs);
static ExcKernelFn exc_kernel(bool noise, bool interf)
{
    static const ExcKernelFn k[2][2] = GPSBB_NI_KERNELS(k_excise);
    return k[noise][interf];
}

extern "C" int gpsbb_device_excise(gpsbb_t *h, const int16_t *d_iq, long nsamp, const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set,
                                   const gpsbb_exc_t *e, const int16_t *hist_in, int16_t *hist_out, int16_t *d_out, uint64_t *clipped,
                                   uint64_t *excised)
{
    ImpairCall ic;
    if (!h || !d_iq || !e || !d_out || (((uintptr_t)d_iq | (uintptr_t)d_out) & 3) || !exc_ok(e, nsamp) || !impair_make(nz, set, (uint64_t)nsamp, &ic))
        return GPSBB_E_BADARG;
    const uintptr_t in0 = (uintptr_t)d_iq, in1 = in0 + 4 * (uintptr_t)nsamp, out0 = (uintptr_t)d_out, out1 = out0 + 4 * (uintptr_t)nsamp;
    if (out0 < in1 && in0 < out1)
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, ic.noise);
    if (rc != GPSBB_OK)
        return rc;
    const int L = e->log2n, N = 1 << L;
    const long nblk = nsamp / (N / 2);
    int run = 0, nwg = 0;
    exc_geometry(L, nblk, &run, &nwg);
    /* ---- scratch, in 8-byte words: the tables of every log2n (uploaded when the buffer is made), the window, the mask in point
     * order, the two histories, the two counts, two counts per workgroup ---- */
    constexpr size_t mask_words = GPSBB_EXC_MAX_N / 64, hist_words = GPSBB_EXC_MAX_N / 2;
    const size_t tab_words = exc_tab_offset(EXC_MAX_LOG2N + 1);
    const size_t o_win = tab_words, o_mask = o_win + win_words, o_hin = o_mask + mask_words, o_hout = o_hin + hist_words, o_cnt = o_hout + hist_words,
                 o_part = o_cnt + 2;
    hipStream_t cs = h->s_compute;
    HIPCHK(h, psd_tab_ready(h));
    if (!h->d_exc.p) {
        HIPCHK(h, (hipError_t)h->d_exc.reserve(o_part + 2 * (size_t)EXC_MAX_WGS));
        std::vector<unsigned long long> t(tab_words + 1); /* (8-byte words: exc_tw is two of them, 16-byte aligned where its offset is even) */
        for (int l = EXC_MIN_LOG2N; l <= EXC_MAX_LOG2N; l++) {
            exc_tw *tw = reinterpret_cast<exc_tw *>(t.data() + exc_tab_offset(l));
            exc_tables(l, psd_table(), psd_table() + PSD_TW, tw, reinterpret_cast<psd_c *>(tw + exc_tw_entries(l)));
        }
        hipError_t er = hipMemcpy(h->d_exc.p, t.data(), tab_words * 8, hipMemcpyHostToDevice);
        for (int n = 0; n < 2 && er == hipSuccess; n++)
            for (int i = 0; i < 2 && er == hipSuccess; i++) /* 80 KB of dynamic LDS at N = 4096: above the 64 KB default limit */
                er = hipFuncSetAttribute(reinterpret_cast<const void *>(exc_kernel(n != 0, i != 0)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)exc_lds_bytes(EXC_MAX_LOG2N));
        if (er != hipSuccess)
            release_all(h->d_exc); /* the tables or no buffer: the next call uploads again */
        HIPCHK(h, er);
    }
    uint32_t maskp[GPSBB_EXC_MAX_N / 32];
    exc_mask_points(e, maskp);
    ExcArgs a;
    memset(&a, 0, sizeof a);
    a.d = iq_view(h, d_iq, 0, ic);
    a.tabs = h->d_tabs.p;
    a.tw = reinterpret_cast<const psd_c *>(h->d_psd_tab.p);
    a.itw = reinterpret_cast<const exc_tw *>(h->d_exc.p + exc_tab_offset(L));
    a.fin = reinterpret_cast<const psd_c *>(a.itw + exc_tw_entries(L));
    int16_t *d_win = reinterpret_cast<int16_t *>(h->d_exc.p + o_win);
    uint32_t *d_mask = reinterpret_cast<uint32_t *>(h->d_exc.p + o_mask), *d_hin = reinterpret_cast<uint32_t *>(h->d_exc.p + o_hin);
    uint32_t *d_hout = reinterpret_cast<uint32_t *>(h->d_exc.p + o_hout);
    a.win = d_win;
    a.maskp = d_mask;
    a.hist_in = d_hin;
    a.hist_out = d_hout;
    a.out = reinterpret_cast<uint32_t *>(d_out);
    a.part = h->d_exc.p + o_part;
    a.thr = e->thr;
    a.nblk = nblk;
    a.run = run;
    a.log2n = L;
    HIPCHK(h, hipMemcpyAsync(d_win, e->win, (size_t)N * sizeof(int16_t), hipMemcpyHostToDevice, cs));
    HIPCHK(h, hipMemcpyAsync(d_mask, maskp, (size_t)N / 8, hipMemcpyHostToDevice, cs));
    if (hist_in)
        HIPCHK(h, hipMemcpyAsync(d_hin, hist_in, (size_t)N * 4, hipMemcpyHostToDevice, cs));
    else
        HIPCHK(h, hipMemsetAsync(d_hin, 0, (size_t)N * 4, cs));
    HIPCHK(h, h->exc_tm.start(cs));
    hipLaunchKernelGGL(exc_kernel(ic.noise, ic.set), dim3((unsigned)nwg), dim3(PSD_WG), exc_lds_bytes(L), cs, a);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_exc_fold, dim3(1), dim3(PSD_WG), 0, cs, a.part, h->d_exc.p + o_cnt, nwg);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->exc_tm.stop(cs));
    std::vector<uint32_t> tail((size_t)N);
    unsigned long long cnt[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(cnt, h->d_exc.p + o_cnt, sizeof cnt, hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipMemcpyAsync(tail.data(), d_hout, (size_t)N * 4, hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipStreamSynchronize(cs));
    if (hist_out)
        memcpy(hist_out, tail.data(), (size_t)N * 4);
    if (clipped)
        *clipped = cnt[0];
    if (excised)
        *excised = cnt[1];
    return GPSBB_OK;
}

/* ---- pulse blanking (include/gpsbb.h gpsbb_device_blank; gpsbb_blank.h, gpsbb_blank.hip.h) ---- */

extern "C" int gpsbb_blank_make(gpsbb_blank_t *b, int win, int pre, int hold, double floor_ms, double thr_db)
{
    return blank_make(b, win, pre, hold, floor_ms, thr_db);
}

extern "C" int gpsbb_blank_from_level(gpsbb_blank_t *b, const gpsbb_level_t *lv, long n, int shift, double thr_db)
{
    return blank_from_level(b, lv, n, shift, thr_db);
}

static int g_blank_nt = 0; /* gpsbb_test_blank_nt (the experiments build): the stores' policy, for tools/blank_rate.py's alternation */

typedef void (*BlankKernelFn)(BlankArgs);
static BlankKernelFn blank_kernel(bool noise, bool interf)
{
    static const BlankKernelFn k[2][2] = GPSBB_NI_KERNELS(k_blank);
    return k[noise][interf];
}

extern "C" int gpsbb_device_blank(gpsbb_t *h, const int16_t *d_iq, long nsamp, const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set,
                                  const gpsbb_blank_t *b, const int16_t *hist_in, int16_t *hist_out, int16_t *d_out, uint64_t *blanked,
                                  uint64_t *triggers)
{
    ImpairCall ic;
    if (!h || !d_iq || !b || !d_out || (((uintptr_t)d_iq | (uintptr_t)d_out) & 3) || nsamp < 1 || !blank_ok(b) ||
        !impair_make(nz, set, (uint64_t)nsamp, &ic))
        return GPSBB_E_BADARG;
    const uintptr_t in0 = (uintptr_t)d_iq, in1 = in0 + 4 * (uintptr_t)nsamp, out0 = (uintptr_t)d_out, out1 = out0 + 4 * (uintptr_t)nsamp;
    if (out0 < in1 && in0 < out1)
        return GPSBB_E_BADARG;
    const int rc = iq_call_begin(h, ic.noise);
    if (rc != GPSBB_OK)
        return rc;
    const int K = blank_hist(b);
    long run = 0, nwg = 0;
    blank_geometry(nsamp, &run, &nwg); /* nwg <= BLANK_MAX_WGS */
    /* ---- scratch, in 8-byte words: the two histories, the two counts, two counts per workgroup ---- */
    constexpr size_t hist_words = (GPSBB_BLANK_MAX_HIST + 1) / 2;
    constexpr size_t o_hin = 0, o_hout = hist_words, o_cnt = 2 * hist_words, o_part = o_cnt + 2;
    hipStream_t cs = h->s_compute;
    HIPCHK(h, (hipError_t)h->d_blank.reserve(o_part + 2 * (size_t)BLANK_MAX_WGS));
    BlankArgs a;
    memset(&a, 0, sizeof a);
    a.d = iq_view(h, d_iq, 0, ic);
    a.tabs = h->d_tabs.p;
    uint32_t *d_hin = reinterpret_cast<uint32_t *>(h->d_blank.p + o_hin), *d_hout = reinterpret_cast<uint32_t *>(h->d_blank.p + o_hout);
    a.hist_in = d_hin;
    a.hist_out = d_hout;
    a.out = reinterpret_cast<uint32_t *>(d_out);
    a.part = h->d_blank.p + o_part;
    a.thr = b->thr;
    a.nsamp = nsamp;
    a.run = run;
    a.L = b->win;
    a.G = b->pre;
    a.hold = b->hold;
    a.K = K;
    a.R = blank_share(b->pre, b->hold);
    a.rcp = ((1u << BLANK_RCP_BITS) + (uint32_t)a.R - 1u) / (uint32_t)a.R;
    a.nt = g_blank_nt;
    if (K > 0) {
        if (hist_in)
            HIPCHK(h, hipMemcpyAsync(d_hin, hist_in, (size_t)K * 4, hipMemcpyHostToDevice, cs));
        else
            HIPCHK(h, hipMemsetAsync(d_hin, 0, (size_t)K * 4, cs));
    }
    HIPCHK(h, h->blank_tm.start(cs));
    hipLaunchKernelGGL(blank_kernel(ic.noise, ic.set), dim3((unsigned)nwg), dim3(BLANK_WG), blank_lds_bytes(K), cs, a);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_exc_fold, dim3(1), dim3(PSD_WG), 0, cs, a.part, h->d_blank.p + o_cnt, (int)nwg);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->blank_tm.stop(cs));
    uint32_t tail[GPSBB_BLANK_MAX_HIST];
    unsigned long long cnt[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(cnt, h->d_blank.p + o_cnt, sizeof cnt, hipMemcpyDeviceToHost, cs));
    if (K > 0)
        HIPCHK(h, hipMemcpyAsync(tail, d_hout, (size_t)K * 4, hipMemcpyDeviceToHost, cs));
    HIPCHK(h, hipStreamSynchronize(cs));
    if (hist_out && K > 0)
        memcpy(hist_out, tail, (size_t)K * 4);
    if (blanked)
        *blanked = cnt[0];
    if (triggers)
        *triggers = cnt[1];
    return GPSBB_OK;
}

extern "C" double gpsbb_cn0_estimate(const gpsbb_corr_t *p, long n, long stride, double seg_seconds)
{
    if (!p || n < 2 || stride < 1 || !(seg_seconds > 0.0) || !std::isfinite(seg_seconds))
        return NAN;
    double mi = 0.0, mq = 0.0;
    for (long k = 0; k < n; k++) {
        mi += (double)p[k * stride].i;
        mq += (double)p[k * stride].q;
    }
    mi /= (double)n;
    mq /= (double)n;
    double vq = 0.0;
    for (long k = 0; k < n; k++) {
        const double d = (double)p[k * stride].q - mq;
        vq += d * d;
    }
    vq /= (double)(n - 1);
    if (!(mi > 0.0) || !(vq > 0.0))
        return NAN;
    return 10.0 * std::log10(mi * mi / (2.0 * seg_seconds * vq));
}

/* iq_out: where the fill's bytes go on the host (nullptr: the device wrote them already); src: where they are in device memory
 * (the render, or its packed form); bytes: how many */
static int fill_block_finish(gpsbb_t *h, gpsbb_batch *b, int nch, int nsamp, int16_t *iq_out, gpsbb_chan_state_t *end_state,
                             const void *src, size_t bytes)
{
    const size_t end_bytes = (size_t)GPSBB_MAX_CHAN * sizeof(gpsbb_chan_state_t);
    HIPCHK(h, (hipError_t)h->h_fill.reserve(end_bytes + 64));
    hipStream_t cs = b->last_cs;
    uint32_t *st = reinterpret_cast<uint32_t *>(h->h_fill.p + end_bytes);
    *st = 0xffffffffu;
    if (GPSBB_KNOB_LONG("GPSBB_FILL_TAIL_KERNEL", 1) != 0) {
        static_assert(sizeof(gpsbb_chan_state_t) % 4 == 0, "copied as 32-bit words");
        hipLaunchKernelGGL(k_fill_tail, dim3(1), dim3(256), 0, cs, end_state ? b->sets[b->last_set].end.p : nullptr, h->d_status.p, h->h_fill.p, nch, st);
        HIPCHK(h, hipGetLastError());
    } else {
        if (end_state)
            HIPCHK(h, hipMemcpyAsync(h->h_fill.p, b->sets[b->last_set].end.p, (size_t)nch * sizeof(gpsbb_chan_state_t), hipMemcpyDeviceToHost, cs));
        HIPCHK(h, hipMemcpyAsync(st, h->d_status.p, 4, hipMemcpyDeviceToHost, cs));
    }
    PUSH_MARK("tail");
    /* (iq_out null: the synthesis kernel wrote into the caller's registered buffer.)  A destination that lies partly in pages a
     * registration pinned is one the runtime's copy refuses (hipErrorInvalidValue): through a pinned buffer of the handle's then */
    bool bounce = false;
    if (iq_out) {
        const uintptr_t page = 4096, a = (uintptr_t)iq_out, e = a + bytes;
        for (const gpsbb::HostReg &r : h->host_regs) {
            const uintptr_t ra = (uintptr_t)r.host & ~(page - 1), re = ((uintptr_t)r.host + r.bytes + page - 1) & ~(page - 1);
            bounce = bounce || (a < re && ra < e);
        }
    }
    if (bounce) {
        HIPCHK(h, (hipError_t)h->h_bounce.reserve(bytes));
        HIPCHK(h, hipMemcpyAsync(h->h_bounce.p, src, bytes, hipMemcpyDeviceToHost, cs));
    } else if (iq_out) {
        HIPCHK(h, hipMemcpyAsync(iq_out, src, bytes, hipMemcpyDeviceToHost, cs));
    }
    PUSH_MARK("iq copy");
    HIPCHK(h, hipStreamSynchronize(cs));
    if (bounce)
        memcpy(iq_out, h->h_bounce.p, bytes);
    if (end_state)
        memcpy(end_state, h->h_fill.p, (size_t)nch * sizeof(gpsbb_chan_state_t));
    if (*st) {
        HIPCHK(h, zero_now(h, h->d_status.p, 4));
        return GPSBB_E_INTERNAL;
    }
    return GPSBB_OK;
}

extern "C" int gpsbb_host_register(gpsbb_t *h, void *ptr, size_t bytes)
{
    if (!h || !ptr || !bytes)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    char *q = static_cast<char *>(ptr);
    for (const gpsbb::HostReg &r : h->host_regs)
        if (q < r.host + r.bytes && r.host < q + bytes)
            return GPSBB_E_STATE; /* overlaps a range that is registered already */
    HIPCHK(h, hipHostRegister(ptr, bytes, hipHostRegisterMapped));
    void *dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dev, ptr, 0);
    if (e != hipSuccess || !dev) {
        (void)hipHostUnregister(ptr);
        h->last_hip = (int)e;
        return GPSBB_E_HIP;
    }
    h->host_regs.push_back({q, static_cast<char *>(dev), bytes});
    return GPSBB_OK;
}

extern "C" int gpsbb_host_unregister(gpsbb_t *h, void *ptr)
{
    if (!h || !ptr)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    for (size_t k = 0; k < h->host_regs.size(); k++)
        if (h->host_regs[k].host == static_cast<char *>(ptr)) {
            /* nothing of a fill is in flight once the call has returned, but a ring's gather or a batch given a pointer into the
             * range may be, on any stream: drain them all before the mapping goes */
            HIPCHK(h, drain_streams(h));
            HIPCHK(h, hipHostUnregister(ptr));
            h->host_regs.erase(h->host_regs.begin() + (long)k);
            return GPSBB_OK;
        }
    return GPSBB_E_STATE;
}

extern "C" int gpsbb_fill_block(gpsbb_t *h, const gpsbb_chan_t *ch, int nch, double delt, int nsamp,
                                int16_t *iq_out, gpsbb_chan_state_t *end_state)
{
    return gpsbb_fill_block_ex(h, ch, nch, delt, nsamp, 0u, iq_out, end_state);
}

/* gpsbb_fill_block_ex, and with ic gpsbb_fill_block_noise / gpsbb_fill_block_impair */
static int fill_block_impl(gpsbb_t *h, const gpsbb_chan_t *ch, int nch, double delt, int nsamp, unsigned flags, const ImpairCall *ic,
                           int16_t *iq_out, gpsbb_chan_state_t *end_state)
{
    if (!h || !ch || !iq_out)
        return GPSBB_E_BADARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->scratch) {
        h->scratch = batch_new(h);
        if (!h->scratch)
            return GPSBB_E_NOMEM;
    }
    gpsbb_batch *b = h->scratch;
    int shift;
    const int fmt = out_format(flags, nsamp, &shift);
    if ((flags & 0xffu & ~GPSBB_FIXED_CARRIER & ~GPSBB_CHAIN_CARRIER) || fmt < 0)
        return GPSBB_E_BADARG;
    const size_t out_bytes = out_block_bytes(fmt, (size_t)nsamp);
    if (ic)
        HIPCHK(h, noise_ready(h));
    g_push_trace.start();
    b->one_stream = GPSBB_KNOB_LONG("GPSBB_FILL_ONE_STREAM", 1) != 0;
    int rc = batch_setup(b, PlanIn{ch, 1, nch, delt, nsamp, flags & GPSBB_FIXED_CARRIER}, plan_opts(h, b->max_sets), b->one_stream ? h->s_compute : h->s_seed);
    if (rc != GPSBB_OK)
        return rc;
    PUSH_MARK("set-up");
    /* iq_out inside a range the caller registered (gpsbb_host_register): the synthesis kernel's stores go there over the bus
     * while it computes, and there is no copy to wait for afterwards */
    int16_t *direct = nullptr;
    for (const gpsbb::HostReg &r : h->host_regs) {
        const char *q = reinterpret_cast<const char *>(iq_out);
        if (q >= r.host && (size_t)(q - r.host) <= r.bytes && out_bytes <= r.bytes - (size_t)(q - r.host)) {
            direct = reinterpret_cast<int16_t *>(r.dev + (q - r.host));
            break;
        }
    }
    /* a packed format: rendered into the handle's buffer, then packed on the same stream — straight into the registered buffer, or
     * into device scratch that is copied out as the int16 block would be */
    /* (with impairments, every format goes this way: k_impair_iq reads the render and writes the bytes that leave) */
    rc = gpsbb_batch_run(b, (fmt || ic) ? nullptr : direct);
    if (rc != GPSBB_OK)
        return rc;
    PUSH_MARK("launches");
    const void *src = b->last_iq;
    if (fmt || ic) {
        void *dst = direct;
        if (!dst) {
            HIPCHK(h, (hipError_t)h->d_pack.reserve(out_bytes));
            dst = h->d_pack.p;
            src = h->d_pack.p;
        }
        HIPCHK(h, out_launch(h, fmt, shift, ic, b->last_iq, dst, (size_t)nsamp * 2, b->last_cs));
    }
    rc = fill_block_finish(h, b, nch, nsamp, direct ? nullptr : iq_out, end_state, src, out_bytes);
    g_push_trace.end();
    return rc;
}

extern "C" int gpsbb_fill_block_ex(gpsbb_t *h, const gpsbb_chan_t *ch, int nch, double delt, int nsamp, unsigned flags,
                                   int16_t *iq_out, gpsbb_chan_state_t *end_state)
{
    return fill_block_impl(h, ch, nch, delt, nsamp, flags, nullptr, iq_out, end_state);
}

extern "C" int gpsbb_fill_block_noise(gpsbb_t *h, const gpsbb_chan_t *ch, int nch, double delt, int nsamp, unsigned flags,
                                      const gpsbb_noise_t *nz, void *iq_out, gpsbb_chan_state_t *end_state)
{
    return gpsbb_fill_block_impair(h, ch, nch, delt, nsamp, flags, nz, nullptr, iq_out, end_state);
}

extern "C" int gpsbb_fill_block_impair(gpsbb_t *h, const gpsbb_chan_t *ch, int nch, double delt, int nsamp, unsigned flags,
                                       const gpsbb_noise_t *nz, const gpsbb_interf_set_t *set, void *iq_out, gpsbb_chan_state_t *end_state)
{
    ImpairCall c;
    if (nsamp < 1 || !impair_make(nz, set, (uint64_t)nsamp, &c))
        return GPSBB_E_BADARG;
    return fill_block_impl(h, ch, nch, delt, nsamp, flags, c.any() ? &c : nullptr, static_cast<int16_t *>(iq_out), end_state);
}

/* the reference's own channel_t[] / gain[] in, rendered, updated in place as its loop leaves them; fixed: the build without
 * FLOAT_CARR_PHASE (h:160-161: a 32-bit accumulator and its step instead of the double) */
static int fill_block_ref(gpsbb_t *h, void *chan, const gpsbb_refchan_layout_t *L, bool fixed, size_t off_step, int max_chan,
                          const double *gain, double delt, int nsamp, int16_t *iq_buff)
{
    if (!h || !chan || !L || !gain || !iq_buff || max_chan < 1 || max_chan > GPSBB_MAX_CHAN ||
        (L->sizeof_dwrd_elem != 4 && L->sizeof_dwrd_elem != 8))
        return GPSBB_E_BADARG;
    gpsbb_chan_t d[GPSBB_MAX_CHAN];
    gpsbb_chan_state_t st[GPSBB_MAX_CHAN];
    char *base = static_cast<char *>(chan);
    auto ld_i = [](const char *p) { int v; memcpy(&v, p, sizeof v); return v; };
    auto ld_u = [](const char *p) { unsigned v; memcpy(&v, p, sizeof v); return v; };
    auto ld_d = [](const char *p) { double v; memcpy(&v, p, sizeof v); return v; };
    for (int i = 0; i < max_chan; i++) {
        const char *c = base + (size_t)i * L->stride;
        memset(&d[i], 0, sizeof d[i]);
        d[i].prn = ld_i(c + L->off_prn);
        if (d[i].prn <= 0) {
            d[i].prn = 0;
            continue;
        }
        d[i].f_carr = ld_d(c + L->off_f_carr);
        d[i].f_code = ld_d(c + L->off_f_code);
        d[i].carr_phase = fixed ? (double)ld_u(c + L->off_carr_phase) : ld_d(c + L->off_carr_phase);
        d[i].code_phase = ld_d(c + L->off_code_phase);
        d[i].iword = ld_i(c + L->off_iword);
        d[i].ibit = ld_i(c + L->off_ibit);
        d[i].icode = ld_i(c + L->off_icode);
        d[i].gain = gain[i];
        for (int k = 0; k < GPSBB_N_DWRD; k++) {
            uint64_t w = 0;
            memcpy(&w, c + L->off_dwrd + (size_t)k * L->sizeof_dwrd_elem, L->sizeof_dwrd_elem);
            d[i].dwrd[k] = (uint32_t)w;
        }
        if (fixed && off_step != (size_t)-1 && std::isfinite(d[i].f_carr) && std::fabs(d[i].f_carr * delt) <= 0.125) {
            /* the step the host computed (c:2675) must be the one the accumulator is advanced by here (c:2748): a host that
             * put anything else into carr_phasestep would get different samples from its own loop */
            const volatile double scaled = 512.0 * 65536.0 * d[i].f_carr * delt;
            if (ld_i(c + off_step) != (int)std::round(scaled))
                return GPSBB_E_BADCHAN;
        }
    }
    int rc = gpsbb_fill_block_ex(h, d, max_chan, delt, nsamp, fixed ? GPSBB_FIXED_CARRIER : 0u, iq_buff, st);
    if (rc != GPSBB_OK)
        return rc;
    for (int i = 0; i < max_chan; i++) {
        if (d[i].prn <= 0)
            continue;
        char *c = base + (size_t)i * L->stride;
        if (fixed) {
            const unsigned ph = (unsigned)st[i].carr_phase; /* the accumulator's value, an integer below 2^32 */
            memcpy(c + L->off_carr_phase, &ph, 4);
        } else {
            memcpy(c + L->off_carr_phase, &st[i].carr_phase, 8);
        }
        memcpy(c + L->off_code_phase, &st[i].code_phase, 8);
        memcpy(c + L->off_iword, &st[i].iword, 4);
        memcpy(c + L->off_ibit, &st[i].ibit, 4);
        memcpy(c + L->off_icode, &st[i].icode, 4);
        memcpy(c + L->off_dataBit, &st[i].dataBit, 4);
        memcpy(c + L->off_codeCA, &st[i].codeCA, 4);
    }
    return GPSBB_OK;
}

extern "C" int gpsbb_fill_block_ref(gpsbb_t *h, void *chan, const gpsbb_refchan_layout_t *L, int max_chan,
                                    const double *gain, double delt, int nsamp, int16_t *iq_buff)
{
    return fill_block_ref(h, chan, L, false, (size_t)-1, max_chan, gain, delt, nsamp, iq_buff);
}

extern "C" int gpsbb_fill_block_ref_fixed(gpsbb_t *h, void *chan, const gpsbb_refchan_layout_t *L, size_t off_carr_phasestep,
                                          int max_chan, const double *gain, double delt, int nsamp, int16_t *iq_buff)
{
    return fill_block_ref(h, chan, L, true, off_carr_phasestep, max_chan, gain, delt, nsamp, iq_buff);
}

/* ================================================================================================== */
/* time-sharded streaming with pinned host gather                                                     */
/* ================================================================================================== */

/* A ring's carrier chain from one push to the next.  A push works on a copy and commits it with one assignment once every enqueue
 * has succeeded; only a move of the carry between the sides — the same state, told the other way — is committed on the spot. */
struct StreamChain {
    ChainCarry carry = {};                     /* IEEE carrier chained on the host across pushes: prn and exact phase */
    /* ... or on the device (gpsbb_stream::d_carry), and then the host keeps: */
    int last_prn[GPSBB_MAX_CHAN] = {0};        /* prn per channel in the last block pushed */
    double rough_phase[GPSBB_MAX_CHAN] = {0};  /* its rough idea of the carrier phase after it */
    bool on_device = false;                    /* where the authoritative carry is right now */
    int fx_prn[GPSBB_MAX_CHAN] = {0};          /* fixed-point carrier: channel state after the last push */
    uint32_t fx_phase[GPSBB_MAX_CHAN] = {0};
    /* The next push does not continue the one before: every channel of its first block starts from its descriptor's phase, as if
     * it had just been allocated (c:1956-1964) — "no satellite was here before" is all the chain has to be told.  phases_too: a
     * ring that starts a new stream (gpsbb_stream_reset) forgets where the old one stood as well. */
    void forget(bool phases_too)
    {
        if (phases_too)
            *this = StreamChain();
        for (int i = 0; i < GPSBB_MAX_CHAN; i++)
            last_prn[i] = fx_prn[i] = carry.prn[i] = 0;
    }
};

struct gpsbb_stream {
    gpsbb *h = nullptr;
    int nch = 0, nsamp = 0, bps = 0, depth = 0;
    double delt = 0.0;
    unsigned flags = 0;
    int fmt = 0, shift = 0; /* output format of the host gather (GPSBB_OUT_*: 0 int16, PACK_SC8, PACK_SC1) */
    bool noise_on = false;  /* gpsbb_stream_set_noise: the gather adds noise (k_impair_iq) ... */
    bool interf_on = false; /* ... gpsbb_stream_set_interf: and the set's J */
    ImpairArgs impair{};    /* their arguments: nz and it each as its setter left it, sample0 = where that call put the stream */
    unsigned long long out_pos = 0; /* the stream position of the next push's first sample */
    struct Slot {
        gpsbb_batch *batch = nullptr;
        PinnedBuf<unsigned char> h_iq;     /* the gather, in the stream's output format (none: GPSBB_STREAM_DEVICE_ONLY) */
        PinnedBuf<unsigned char> h_end;    /* the end states, and the status word behind them */
        PinnedBuf<unsigned long long> h_dig; /* on the first GPSBB_PUSH_DIGEST: the push's block digests */
        bool has_dig = false;
        DevBuf<LevelOut> d_lvl;            /* on the first GPSBB_PUSH_LEVEL: the push's block levels on the device ... */
        PinnedBuf<LevelOut> h_lvl;         /* ... and pinned, behind the gather on its stream */
        bool has_lvl = false;
        Event computed, copied;
        void release()
        {
            if (batch)
                gpsbb_batch_destroy(batch);
            batch = nullptr;
            release_all(h_iq, h_dig, h_lvl, d_lvl, h_end, computed, copied);
        }
    };
    std::vector<Slot> slots;
    uint64_t head = 0, tail = 0; /* pushes / pops so far */
    StreamChain chain;           /* where the carrier chain stands after the last push */
    DevBuf<ChainCarryDev> d_carry; /* the carry while it is on the device (gpsbb_walk.hip.h): the exact phase never leaves it */
    Event ev_prefix, ev_fix;       /* ... and what orders its users across pushes: all three or none (push_carry_to_device) */
    std::vector<gpsbb_chan_t> seeded; /* a host-side push: its descriptors with every block's start phase */
    std::vector<double> seeds;
    bool poisoned = false; /* a push failed after part of it had been enqueued: the chain's state on the device has
                              moved on without the host's; nothing more can be pushed or popped */
};

extern "C" void gpsbb_stream_destroy(gpsbb_stream_t *s)
{
    if (!s)
        return;
    (void)hipSetDevice(s->h->device);
    (void)drain_streams(s->h); /* the carry, the pinned slots and the events: pre-pass, synthesis and copy streams hold work on them */
    release_all(s->d_carry, s->ev_prefix, s->ev_fix);
    for (auto &sl : s->slots)
        sl.release();
    delete s;
}

extern "C" int gpsbb_stream_create(gpsbb_t *h, int nch, double delt, int nsamp, int blocks_per_slot,
                                   int depth, unsigned flags, gpsbb_stream_t **out)
{
    if (!h || !out || nch < 1 || nch > GPSBB_MAX_CHAN || nsamp < 1 || blocks_per_slot < 1 || depth < 2 ||
        depth > 64 || !(delt > 0.0) || (flags & 0xffu & ~(GPSBB_CHAIN_CARRIER | GPSBB_FIXED_CARRIER | GPSBB_STREAM_DEVICE_ONLY)))
        return GPSBB_E_BADARG;
    int shift;
    const int fmt = out_format(flags, nsamp, &shift);
    if (fmt < 0 || (fmt && (flags & GPSBB_STREAM_DEVICE_ONLY))) /* the slots in HBM stay int16 */
        return GPSBB_E_BADARG;
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    gpsbb_stream *s = new (std::nothrow) gpsbb_stream;
    if (!s)
        return GPSBB_E_NOMEM;
    s->h = h;
    s->nch = nch;
    s->nsamp = nsamp;
    s->bps = blocks_per_slot;
    s->depth = depth;
    s->delt = delt;
    s->flags = flags;
    s->fmt = fmt;
    s->shift = shift;
    s->slots.resize(depth);
    const size_t iq_bytes = (size_t)blocks_per_slot * nsamp * 4;
    const size_t host_bytes = (size_t)blocks_per_slot * out_block_bytes(fmt, (size_t)nsamp);
    const size_t end_bytes = (size_t)blocks_per_slot * nch * sizeof(gpsbb_chan_state_t);
    for (auto &sl : s->slots) {
        sl.batch = batch_new(h);
        hipError_t e = sl.batch ? hipSuccess : hipErrorOutOfMemory;
        if (e == hipSuccess && ((&sl - &s->slots[0]) & 1))
            e = use_second_seed_stream(sl.batch);
        if (e == hipSuccess) sl.batch->max_sets = 1; /* consecutive pushes use different slots: one table set each */
        if (e == hipSuccess) e = (hipError_t)sl.batch->d_iq.reserve(iq_bytes / 2);
        if (e == hipSuccess && !(flags & GPSBB_STREAM_DEVICE_ONLY))
            e = (hipError_t)sl.h_iq.reserve(host_bytes);
        if (e == hipSuccess) e = (hipError_t)sl.h_end.reserve(end_bytes + 32); /* + the status word */
        if (e == hipSuccess) e = sl.computed.make(hipEventDisableTiming);
        if (e == hipSuccess) e = sl.copied.make(hipEventDisableTiming);
        if (e != hipSuccess) {
            h->last_hip = (int)e;
            gpsbb_stream_destroy(s);
            return e == hipErrorOutOfMemory ? GPSBB_E_NOMEM : GPSBB_E_HIP;
        }
    }
    *out = s;
    return GPSBB_OK;
}

extern "C" int gpsbb_stream_pending(const gpsbb_stream_t *s) { return s ? (int)(s->head - s->tail) : 0; }

extern "C" int gpsbb_stream_reset(gpsbb_stream_t *s)
{
    if (!s)
        return GPSBB_E_BADARG;
    if (s->poisoned || s->head != s->tail)
        return GPSBB_E_STATE;
    gpsbb *h = s->h;
    HIPCHK(h, hipSetDevice(h->device));
    /* everything the last stream left in the queues has completed (its slots were popped), but the chain kernels of its
     * last push may still be writing the carry: wait for the handle before touching it */
    const int rc = gpsbb_sync(h);
    if (rc != GPSBB_OK)
        return rc;
    if (s->d_carry.p)
        HIPCHK(h, zero_now(h, s->d_carry.p, sizeof(ChainCarryDev)));
    s->chain.forget(true);
    s->head = s->tail = 0;
    s->out_pos = s->noise_on || !s->interf_on ? s->impair.nz.sample0 : s->impair.it.sample0;
    return GPSBB_OK;
}

extern "C" int gpsbb_stream_set_noise(gpsbb_stream_t *s, const gpsbb_noise_t *nz)
{
    if (!s || (s->flags & GPSBB_STREAM_DEVICE_ONLY))
        return GPSBB_E_BADARG;
    if (!nz) {
        s->noise_on = false;
        return GPSBB_OK;
    }
    NoiseArgs a;
    if (!noise_args(nz, &a))
        return GPSBB_E_BADARG;
    if (s->interf_on && (a.sample0 != s->impair.it.sample0 || a.shift != s->impair.it.shift))
        return GPSBB_E_BADARG; /* (the later of the two calls checks the rule) */
    HIPCHK(s->h, hipSetDevice(s->h->device));
    HIPCHK(s->h, noise_ready(s->h));
    s->impair.nz = a;
    s->out_pos = a.sample0;
    s->noise_on = true;
    return GPSBB_OK;
}

extern "C" int gpsbb_stream_set_interf(gpsbb_stream_t *s, const gpsbb_interf_set_t *set)
{
    if (!s || (s->flags & GPSBB_STREAM_DEVICE_ONLY))
        return GPSBB_E_BADARG;
    if (!set) {
        s->interf_on = false;
        return GPSBB_OK;
    }
    InterfArgs a;
    if (!interf_args(set, &a) || !interf_at(&a, set->sample0, (uint64_t)s->bps * (uint64_t)s->nsamp))
        return GPSBB_E_BADARG;
    if (s->noise_on && (s->impair.nz.sample0 != a.sample0 || s->impair.nz.shift != a.shift))
        return GPSBB_E_BADARG;
    HIPCHK(s->h, hipSetDevice(s->h->device));
    HIPCHK(s->h, noise_ready(s->h));
    s->impair.it = a;
    s->out_pos = a.sample0;
    s->interf_on = true;
    return GPSBB_OK;
}

extern "C" int gpsbb_stream_timing_stats(gpsbb_stream_t *s, int *nruns, float *ms_seed_sum, float *ms_synth_sum, int reset)
{
    if (!s)
        return GPSBB_E_BADARG;
    int n = 0;
    float a = 0, c = 0;
    for (auto &sl : s->slots) {
        int k = 0;
        float x = 0, y = 0, z = 0;
        const int rc = gpsbb_batch_timing_stats(sl.batch, &k, &x, &y, &z, reset);
        if (rc != GPSBB_OK)
            return rc;
        n += k;
        a += x;
        c += y;
    }
    if (nruns) *nruns = n;
    if (ms_seed_sum) *ms_seed_sum = a;
    if (ms_synth_sum) *ms_synth_sum = c;
    return GPSBB_OK;
}

static int stream_push(gpsbb_stream_t *s, const gpsbb_chan_t *ch, bool new_chain, bool want_digest, bool want_level);

extern "C" int gpsbb_stream_push(gpsbb_stream_t *s, const gpsbb_chan_t *ch) { return stream_push(s, ch, false, false, false); }

extern "C" int gpsbb_stream_push_ex(gpsbb_stream_t *s, const gpsbb_chan_t *ch, unsigned flags)
{
    if (flags & ~(GPSBB_PUSH_NEW_CHAIN | GPSBB_PUSH_DIGEST | GPSBB_PUSH_LEVEL))
        return GPSBB_E_BADARG;
    if ((flags & GPSBB_PUSH_LEVEL) && ((flags & GPSBB_PUSH_DIGEST) || (s && (s->flags & GPSBB_STREAM_DEVICE_ONLY))))
        return GPSBB_E_BADARG; /* (measured on the gather's stream: a ring without one, or a push whose digests ride elsewhere) */
    return stream_push(s, ch, (flags & GPSBB_PUSH_NEW_CHAIN) != 0, (flags & GPSBB_PUSH_DIGEST) != 0, (flags & GPSBB_PUSH_LEVEL) != 0);
}

/* what the next push's gather and measurement are given: the ring's noise and set, whichever are on, at its position; false: with a
 * set, the push would reach position 2^63 */
static bool stream_impair(const gpsbb_stream *s, ImpairCall *c)
{
    memset(c, 0, sizeof *c);
    c->noise = s->noise_on;
    c->set = s->interf_on;
    if (s->noise_on)
        c->a.nz = s->impair.nz;
    if (s->interf_on) {
        c->a.it = s->impair.it;
        c->a.nz.shift = s->impair.it.shift;
    }
    return impair_at(c, s->out_pos, (uint64_t)s->bps * (uint64_t)s->nsamp);
}

/* GPSBB_PUSH_LEVEL: what k_level will be given is checked, and its memory made, before anything of the push exists */
static int push_level_memory(gpsbb_stream *s, const ImpairCall &ic)
{
    if (!level_fits(ic.a, ic.noise, s->nsamp))
        return GPSBB_E_BADARG;
    auto &sl = s->slots[s->head % s->depth];
    HIPCHK(s->h, hipSetDevice(s->h->device));
    HIPCHK(s->h, (hipError_t)sl.d_lvl.reserve((size_t)s->bps));
    HIPCHK(s->h, (hipError_t)sl.h_lvl.reserve((size_t)s->bps));
    return GPSBB_OK;
}

/* A device-side push: the carry in device memory, made on the first such push, moved there behind a host-side one; `next` follows. */
static int push_carry_to_device(gpsbb_stream *s, StreamChain &next)
{
    gpsbb *h = s->h;
    StreamChain &at = s->chain;
    if (!s->ev_fix) { /* the last of the four steps: there only once all of them have succeeded */
        hipError_t e = (hipError_t)s->d_carry.reserve(1);
        e = e ? e : zero_now(h, s->d_carry.p, sizeof(ChainCarryDev));
        e = e ? e : s->ev_prefix.make(hipEventDisableTiming);
        e = e ? e : s->ev_fix.make(hipEventDisableTiming);
        if (e != hipSuccess) /* all or none (FixScratch::reserve): a carry without its events would be used unordered, and maybe unzeroed */
            release_all(s->d_carry, s->ev_prefix, s->ev_fix);
        HIPCHK(h, e);
    }
    if (!at.on_device && s->head > 0) {
        /* host -> device: the exact phases as both the prediction and the truth */
        ChainCarryDev c;
        for (int i = 0; i < GPSBB_MAX_CHAN; i++)
            c.approx_end[i] = c.exact_end[i] = at.carry.phase[i];
        const int rc = gpsbb_sync(h);
        if (rc != GPSBB_OK)
            return rc;
        HIPCHK(h, hipMemcpy(s->d_carry.p, &c, sizeof c, hipMemcpyHostToDevice));
        HIPCHK(h, hipStreamSynchronize(nullptr)); /* (see zero_now) */
        for (int i = 0; i < s->nch; i++) {
            at.last_prn[i] = at.carry.prn[i];
            at.rough_phase[i] = at.carry.phase[i];
        }
    }
    at.on_device = true;
    next = at;
    return GPSBB_OK;
}

/* A host-side push: the carry fetched from the device behind a device-side one, the chain resolved on host threads into next.carry,
 * and the push goes on as one of independent blocks: `in` takes descriptors that carry every block's start phase, and no plan begun. */
static int push_carry_to_host(gpsbb_stream *s, StreamChain &next, PlanIn &in, PushSide &side)
{
    gpsbb *h = s->h;
    StreamChain &at = s->chain;
    if (at.on_device) {
        /* device -> host */
        ChainCarryDev c;
        const int rc = gpsbb_sync(h);
        if (rc != GPSBB_OK)
            return rc;
        HIPCHK(h, hipMemcpy(&c, s->d_carry.p, sizeof c, hipMemcpyDeviceToHost));
        for (int i = 0; i < s->nch; i++) {
            at.carry.prn[i] = at.last_prn[i];
            at.carry.phase[i] = c.exact_end[i];
        }
        at.on_device = false;
    }
    next = at;
    const size_t nbc = (size_t)s->bps * s->nch;
    s->seeded.assign(in.ch, in.ch + nbc);
    s->seeds.resize(nbc);
    chain_carrier_host(in.ch, s->bps, s->nch, s->delt, s->nsamp, s->seeds.data(), 0, &next.carry);
    for (size_t k = 0; k < nbc; k++)
        s->seeded[k].carr_phase = s->seeds[k];
    in.ch = s->seeded.data();
    in.flags &= ~GPSBB_CHAIN_CARRIER;
    side.begun = false;
    return GPSBB_OK;
}

/* Everything behind the synthesis of a push: the gather, the end states, the digests, the level, and the event a pop waits for. */
static int push_outputs(gpsbb_stream *s, gpsbb_stream::Slot &sl, ImpairCall &ic, bool want_digest, bool want_level)
{
    gpsbb *h = s->h;
    gpsbb_batch *b = sl.batch;
    /* Host-bound output: gather on the copy stream — pinned, asynchronous, overlaps the next push's kernels.  A device-only
     * ring has none: its end states (and digests) merely follow the synthesis, so they ride behind it on its stream, with no
     * event wait and no stream that holds one (a hardware queue whose head is a wait for a 1.5 ms kernel runs nothing that
     * shares it until then).  (The slot's previous D2H copy was waited for by the pop that freed it.) */
    hipStream_t cs = b->last_cs;
    if (sl.h_iq.p) {
        if (!h->s_copy)
            HIPCHK(h, hipStreamCreateWithFlags(&h->s_copy, hipStreamNonBlocking));
        cs = h->s_copy;
        HIPCHK(h, hipStreamWaitEvent(cs, b->last_done, 0));
    }
    PUSH_MARK("wait");
    if (sl.h_iq.p) {
        const bool sdma = GPSBB_KNOB_SET("GPSBB_GATHER_SDMA"); /* experiment: the runtime's copy instead */
        if (sdma && !ic.any() && !s->fmt) {
            HIPCHK(h, hipMemcpyAsync(sl.h_iq.p, b->d_iq.p, (size_t)s->bps * s->nsamp * 4, hipMemcpyDeviceToHost, cs));
        } else {
            /* the plain gather, packed, or with noise and interference on the way out: the same launch that returns at once */
            HIPCHK(h, out_launch(h, s->fmt, s->shift, ic.any() ? &ic : nullptr, b->d_iq.p, sl.h_iq.p, (size_t)s->bps * s->nsamp * 2, cs));
        }
    }
    PUSH_MARK("iq");
    /* end states (40 B each: a multiple of 16 bytes for any even count; odd counts are rounded up into the
     * allocation's slack) + the self-check word, by a small kernel: see k_end_states_to_host */
    const size_t bytes = (size_t)s->bps * s->nch * sizeof(gpsbb_chan_state_t);
    hipLaunchKernelGGL(k_end_states_to_host, dim3(64), dim3(256), 0, cs, (const uint4 *)b->sets[b->last_set].end.p,
                       (uint4 *)sl.h_end.p, (bytes + 15) / 16, h->d_status.p, (uint32_t *)(sl.h_end.p + ((bytes + 15) & ~(size_t)15)));
    HIPCHK(h, hipGetLastError());
    if (want_digest) {
        HIPCHK(h, hipMemcpyAsync(sl.h_dig.p, b->d_dig.p, (size_t)s->bps * sizeof(unsigned long long), hipMemcpyDeviceToHost, cs));
        sl.has_dig = true;
    }
    if (want_level) {
        /* the slot measured where it is gathered: behind the gather, on its stream, results through pinned memory */
        HIPCHK(h, level_launch(h, ic.a, ic.noise, b->d_iq.p, s->bps, s->nsamp, sl.d_lvl.p, cs));
        HIPCHK(h, hipMemcpyAsync(sl.h_lvl.p, sl.d_lvl.p, (size_t)s->bps * sizeof(LevelOut), hipMemcpyDeviceToHost, cs));
        sl.has_lvl = true;
    }
    PUSH_MARK("endst");
    HIPCHK(h, hipEventRecord(sl.copied, cs));
    return GPSBB_OK;
}

/* What ends with a push, however it ends: the slot's batch holds the link for the length of the push (set-up and launch read it).
 * And once `queued` — kernels of the push may be in the queues; with the device-side chain they advance the carry in device
 * memory — a failure leaves the host's and the device's view of the stream apart: the stream is closed instead of letting a retry
 * chain from the wrong phase.  Before that a failure just returns: a NEW_CHAIN taken and a carry moved stay, nothing else does. */
struct PushGuard {
    gpsbb_stream *s;
    gpsbb_batch *b;
    bool queued = false, done = false;
    ~PushGuard()
    {
        b->link = StreamLink();
        s->poisoned = s->poisoned || (queued && !done);
    }
};

/* Blocks consecutive in time with the IEEE carrier: the carrier phase carries over from block to block and from push to push,
 * exactly; on which side is decided per push (plan_push_side). */
static int stream_push(gpsbb_stream_t *s, const gpsbb_chan_t *ch, bool new_chain, bool want_digest, bool want_level)
{
    if (!s || !ch)
        return GPSBB_E_BADARG;
    if (s->poisoned || s->head - s->tail >= (uint64_t)s->depth)
        return GPSBB_E_STATE; /* ring full: pop first */
    ImpairCall ic; /* the one value the gather and k_level are both given */
    if (!stream_impair(s, &ic))
        return GPSBB_E_BADARG; /* the push would reach position 2^63 */
    int rc = want_level ? push_level_memory(s, ic) : GPSBB_OK;
    if (rc != GPSBB_OK)
        return rc;
    if (new_chain)
        s->chain.forget(false);
    gpsbb *h = s->h;
    g_push_trace.start();
    HIPCHK(h, hipSetDevice(h->device));
    auto &sl = s->slots[s->head % s->depth];
    gpsbb_batch *b = sl.batch;
    const PlanOpts opts = plan_opts(h, b->max_sets);
    PlanIn in{ch, s->bps, s->nch, s->delt, s->nsamp, s->flags & (GPSBB_CHAIN_CARRIER | GPSBB_FIXED_CARRIER)};
    PushSide side;
    rc = plan_push_side(side, b->img, in, opts);
    if (rc != GPSBB_OK)
        return rc;
    StreamChain next = s->chain; /* the chain behind this push */
    if (side.chain == PUSH_CHAIN_DEVICE)
        rc = push_carry_to_device(s, next);
    else if (side.chain == PUSH_CHAIN_HOST)
        rc = push_carry_to_host(s, next, in, side);
    if (rc != GPSBB_OK)
        return rc;
    /* what the push lends the batch: the carry, its events and the chain as the push found it (the rough phases in and out, in
     * the copy); the accumulator's chaining state behind a first push */
    PushGuard guard{s, b};
    if (side.chain == PUSH_CHAIN_DEVICE) {
        b->link.d_carry = s->d_carry.p;
        b->link.carry_prn = s->chain.last_prn;
        b->link.carry_phase = next.rough_phase;
        b->link.ev_prefix = s->ev_prefix;
        b->link.ev_fix = s->ev_fix;
        b->link.stream_turn = (unsigned)s->head;
    }
    if ((s->flags & GPSBB_FIXED_CARRIER) && (s->flags & GPSBB_CHAIN_CARRIER) && s->head > 0) {
        b->link.fixed_prev_prn = s->chain.fx_prn;
        b->link.fixed_prev_phase = s->chain.fx_phase;
    }
    PUSH_MARK("plan");
    /* descriptors and plans go up on the stream that will run this push's pre-pass */
    hipStream_t us = nullptr;
    HIPCHK(h, batch_prepass_stream(b, b->link.d_carry != nullptr, &us));
    rc = batch_setup(b, in, opts, us, side.begun ? &side.plan0 : nullptr);
    PUSH_MARK("setup");
    if (rc != GPSBB_OK)
        return rc;
    for (int i = 0; i < s->nch; i++) {
        const size_t k = (size_t)(s->bps - 1) * s->nch + i;
        if (side.chain == PUSH_CHAIN_DEVICE)
            next.last_prn[i] = in.ch[k].prn > 0 ? in.ch[k].prn : 0;
        if (s->flags & GPSBB_FIXED_CARRIER) {
            next.fx_prn[i] = in.ch[k].prn > 0 ? in.ch[k].prn : 0;
            next.fx_phase[i] = b->img.h_kph0[k] + (uint32_t)s->nsamp * (uint32_t)b->img.h_kstep[k];
        }
    }
    b->last_iq = b->d_iq.p;
    guard.queued = true;
    b->want_digest = want_digest;
    if (want_digest)
        HIPCHK(h, (hipError_t)sl.h_dig.reserve((size_t)s->bps));
    sl.has_dig = false;
    sl.has_lvl = false;
    rc = batch_launch(b, b->d_iq.p);
    PUSH_MARK("launch");
    if (rc != GPSBB_OK)
        return rc;
    PUSH_MARK("rec");
    rc = push_outputs(s, sl, ic, want_digest, want_level);
    if (rc != GPSBB_OK)
        return rc;
    s->chain = next; /* every enqueue of this push has succeeded: the chain moves on */
    if (s->noise_on || s->interf_on)
        s->out_pos += (unsigned long long)s->bps * (unsigned long long)s->nsamp;
    s->head++;
    guard.done = true;
    g_push_trace.end();
    return GPSBB_OK;
}

extern "C" int gpsbb_stream_pop(gpsbb_stream_t *s, const int16_t **iq, gpsbb_chan_state_t *end_state)
{
    return gpsbb_stream_pop_digest(s, iq, end_state, nullptr);
}

static int stream_pop(gpsbb_stream_t *s, const int16_t **iq, gpsbb_chan_state_t *end_state, uint64_t *digests, gpsbb_level_t *levels);

extern "C" int gpsbb_stream_pop_digest(gpsbb_stream_t *s, const int16_t **iq, gpsbb_chan_state_t *end_state, uint64_t *digests)
{
    return stream_pop(s, iq, end_state, digests, nullptr);
}

extern "C" int gpsbb_stream_pop_level(gpsbb_stream_t *s, const int16_t **iq, gpsbb_chan_state_t *end_state, gpsbb_level_t *levels)
{
    return stream_pop(s, iq, end_state, nullptr, levels);
}

static int stream_pop(gpsbb_stream_t *s, const int16_t **iq, gpsbb_chan_state_t *end_state, uint64_t *digests, gpsbb_level_t *levels)
{
    if (!s || !iq)
        return GPSBB_E_BADARG;
    if (s->poisoned || s->head == s->tail)
        return GPSBB_E_STATE;
    if (digests && !s->slots[s->tail % s->depth].has_dig)
        return GPSBB_E_STATE; /* the slot was not pushed with GPSBB_PUSH_DIGEST */
    if (levels && !s->slots[s->tail % s->depth].has_lvl)
        return GPSBB_E_STATE; /* ... nor with GPSBB_PUSH_LEVEL */
    gpsbb *h = s->h;
    HIPCHK(h, hipSetDevice(h->device));
    auto &sl = s->slots[s->tail % s->depth];
    HIPCHK(h, hipEventSynchronize(sl.copied));
    *iq = sl.h_iq.p ? reinterpret_cast<const int16_t *>(sl.h_iq.p) : sl.batch->d_iq.p; /* GPSBB_STREAM_DEVICE_ONLY: the slot's buffer in HBM */
    if (end_state)
        memcpy(end_state, sl.h_end.p, (size_t)s->bps * s->nch * sizeof(gpsbb_chan_state_t));
    if (digests)
        memcpy(digests, sl.h_dig.p, (size_t)s->bps * sizeof(unsigned long long));
    if (levels)
        memcpy(levels, sl.h_lvl.p, (size_t)s->bps * sizeof(gpsbb_level_t));
    s->tail++;
    uint32_t st = 0;
    memcpy(&st, sl.h_end.p + (((size_t)s->bps * s->nch * sizeof(gpsbb_chan_state_t) + 15) & ~(size_t)15), 4);
    if (st) {
        HIPCHK(h, zero_now(h, h->d_status.p, 4));
        return GPSBB_E_INTERNAL;
    }
    return GPSBB_OK;
}

/* ================================================================================================== */
/* host helpers                                                                                       */
/* ================================================================================================== */

extern "C" int gpsbb_device_affinity(int device, int *numa_node, char *cpulist, size_t cpulist_cap)
{
    if (device < 0)
        return GPSBB_E_BADARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count)
        return GPSBB_E_NODEVICE;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess)
        return GPSBB_E_HIP;
    for (char *c = bdf; *c; c++)
        *c = (char)tolower((unsigned char)*c); /* sysfs spells the address in lower case */
    if (numa_node)
        *numa_node = -1;
    if (cpulist && cpulist_cap)
        cpulist[0] = 0;
    char path[160];
    if (numa_node) {
        snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
        if (FILE *f = fopen(path, "r")) {
            int v = -1;
            if (fscanf(f, "%d", &v) == 1)
                *numa_node = v;
            fclose(f);
        }
    }
    if (cpulist && cpulist_cap) {
        snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bdf);
        if (FILE *f = fopen(path, "r")) {
            if (fgets(cpulist, (int)cpulist_cap, f)) {
                size_t n = strlen(cpulist);
                while (n && (cpulist[n - 1] == '\n' || cpulist[n - 1] == ' '))
                    cpulist[--n] = 0;
            } else {
                cpulist[0] = 0;
            }
            fclose(f);
        }
    }
    return GPSBB_OK;
}

static void chain_carrier_host(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp, double *seed,
                               int nthreads, ChainCarry *carry)
{
    auto work = [&](int i0, int i1) {
        for (int i = i0; i < i1; i++) {
            int prev_prn = carry ? carry->prn[i] : 0;
            double prev_x = carry ? carry->phase[i] : 0.0;
            for (int b = 0; b < nblocks; b++) {
                const gpsbb_chan_t &c = ch[(size_t)b * nch + i];
                double x0 = (c.prn > 0 && c.prn == prev_prn) ? prev_x : c.carr_phase;
                seed[(size_t)b * nch + i] = c.prn > 0 ? x0 : 0.0;
                if (c.prn > 0) {
                    volatile double s = c.f_carr * delt; /* rounded on its own, as in the loop */
                    prev_x = carr_jump(x0, s, nsamp);
                }
                prev_prn = c.prn > 0 ? c.prn : 0;
            }
            if (carry) {
                carry->prn[i] = prev_prn;
                carry->phase[i] = prev_x;
            }
        }
    };
    if (nthreads <= 0 || nthreads > nch)
        nthreads = nch;
    if (nthreads == 1)
        work(0, nch);
    else
        channel_threads(nch, nthreads, work);
}

extern "C" int gpsbb_chain_carrier_host(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp,
                                        double *seed, int nthreads)
{
    if (!ch || !seed || nblocks < 1 || nch < 1 || nch > GPSBB_MAX_CHAN || nsamp < 1 || !(delt > 0.0))
        return GPSBB_E_BADARG;
    for (size_t k = 0; k < (size_t)nblocks * nch; k++)
        if (!chan_ok(ch[k], delt))
            return GPSBB_E_BADCHAN;
    chain_carrier_host(ch, nblocks, nch, delt, nsamp, seed, nthreads, nullptr);
    return GPSBB_OK;
}

/* ---- the carrier chain alone, on the device ---------------------------------------------------------- */

/* What gpsbb_chain_carrier keeps between calls: its plan and host images (plan_chain_only), and its device scratch — 24-byte chain
 * descriptors, rough start phases, the chain's per-block record and the carry from one sub-batch to the next.  Nothing of a
 * synthesis batch (rows, tile states, IQ) exists here. */
struct ChainOnly {
    ChainOnlyPlan plan;
    PlanImages img; /* h_cd, h_start0 of all the call's blocks; the row walks read every block's exact start phase back into h_cd */
    DevBuf<ChainDesc> d_cd;
    DevBuf<double> d_start0;
    DevBuf<ChainAux> d_aux;
    DevBuf<ChainCarryDev> d_carry;
    DevBuf<uint32_t> d_status; /* a self-check word of its own: the handle's may belong to a push still in flight */
    FixScratch fix;
    /* the lap-parallel chain (gpsbb_laps.hip.h with nothing to emit): the phase after every block, scratch of the lap kernels */
    DevBuf<double> d_lap_end;
    LapScratch lap;
    DevBuf<unsigned long long> d_hz_scratch; /* (a chain alone counts no hazards: the render of those blocks does) */
    std::vector<double> h_lap_end;
};

static void chain_only_free(gpsbb *h)
{
    ChainOnly *c = h->chain_only;
    if (!c)
        return;
    release_all(c->d_cd, c->d_start0, c->d_aux, c->d_lap_end, c->lap, c->fix, c->d_hz_scratch, c->d_carry, c->d_status);
    delete c;
    h->chain_only = nullptr;
}

/* The scratch every piece shares, cleared: the carry from piece to piece, the self-check word, the lap kernels' hazard counters. */
static int chain_only_scratch(gpsbb *h, ChainOnly *c, size_t lap_seeds)
{
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, (hipError_t)c->d_carry.reserve(1));
    HIPCHK(h, (hipError_t)c->d_status.reserve(1));
    HIPCHK(h, hipMemsetAsync(c->d_carry.p, 0, sizeof(ChainCarryDev), h->s_seed));
    HIPCHK(h, hipMemsetAsync(c->d_status.p, 0, 4, h->s_seed));
    if (c->plan.laps) {
        HIPCHK(h, (hipError_t)c->d_hz_scratch.reserve(8));
        HIPCHK(h, hipMemsetAsync(c->d_hz_scratch.p, 0, c->d_hz_scratch.cap * sizeof *c->d_hz_scratch.p, h->s_seed));
        if (lap_seeds)
            c->h_lap_end.resize(lap_seeds);
    }
    return GPSBB_OK;
}

/* What the chain kernels see of a piece, whichever pre-pass walks it: the chain descriptors alone, the carry from the piece
 * before, and which channels of its first block go on from the block before it. */
static BatchDev chain_only_dev(const ChainOnly *c, const ChainOnlyPiece &pc, const PlanIn &in, unsigned long long *hazards)
{
    BatchDev p;
    memset(&p, 0, sizeof p);
    p.nblocks = pc.nb;
    p.nch = in.nch;
    p.nsamp = in.nsamp;
    p.ntiles = (in.nsamp + TILE - 1) / TILE;
    p.nstates = p.ntiles;
    p.delt = in.delt;
    p.flags = GPSBB_CHAIN_CARRIER;
    p.status = c->d_status.p;
    p.hazards = hazards;
    p.chain_dev = 1;
    p.nseg = 1;
    p.nvb = pc.nb;
    p.cd = c->d_cd.p;
    p.carry = c->d_carry.p;
    p.cont0_mask = pc.cont0_mask;
    return p;
}

/* One piece by the lap-parallel pre-pass (gpsbb_laps.hip.h: plan, reference walks, scan, true walks with nothing to emit but the
 * phase after every block, repair); want_seeds: those phases brought back into h_lap_end. */
static int chain_only_lap_piece(gpsbb *h, ChainOnly *c, const ChainOnlyPiece &pc, const PlanIn &in, bool want_seeds)
{
    hipStream_t ss = h->s_seed;
    const size_t nbc = (size_t)pc.nb * in.nch, k0 = (size_t)pc.b0 * in.nch;
    HIPCHK(h, (hipError_t)c->d_cd.reserve(nbc));
    HIPCHK(h, (hipError_t)c->d_lap_end.reserve(nbc));
    HIPCHK(h, (hipError_t)c->lap.reserve(nbc, (size_t)in.nch, (size_t)pc.nb, pc.chunk0[1][in.nch], false));
    HIPCHK(h, hipMemcpyAsync(c->d_cd.p, c->img.h_cd.data() + k0, nbc * sizeof(ChainDesc), hipMemcpyHostToDevice, ss));
    LapDev L;
    c->lap.dev(L);
    lap_dev_plan(L, pc.chunk0, true, nbc);
    BatchDev p = chain_only_dev(c, pc, in, c->d_hz_scratch.p);
    p.lap_end = c->d_lap_end.p;
    lap_chain_launch(ss, p, L, in.nch, NCO_CARR, lap_pass2_kernel(NCO_CARR, false, 0));
    HIPCHK(h, hipGetLastError());
    if (want_seeds)
        HIPCHK(h, hipMemcpyAsync(c->h_lap_end.data() + k0, c->d_lap_end.p, nbc * sizeof(double), hipMemcpyDeviceToHost, ss));
    HIPCHK(h, hipStreamSynchronize(ss));
    return GPSBB_OK;
}

/* One piece by the row walks (gpsbb_walk.hip.h: pass A, prefix, pass B, k_chain_fix_par); want_seeds: the exact start phase of
 * every block, as k_chain_fix_par left it in the chain descriptors, brought back over the piece's part of h_cd. */
static int chain_only_walk_piece(gpsbb *h, ChainOnly *c, const ChainOnlyPiece &pc, const PlanIn &in, bool want_seeds)
{
    hipStream_t ss = h->s_seed;
    const size_t nbc = (size_t)pc.nb * in.nch, k0 = (size_t)pc.b0 * in.nch;
    HIPCHK(h, (hipError_t)c->d_cd.reserve(nbc));
    HIPCHK(h, (hipError_t)c->d_start0.reserve(nbc));
    HIPCHK(h, (hipError_t)c->d_aux.reserve(nbc));
    HIPCHK(h, c->fix.reserve((size_t)GPSBB_MAX_CHAN * ((CHAIN_ONLY_BLOCKS + FIXP_WG_ALONE - 1) / FIXP_WG_ALONE), ss));
    HIPCHK(h, hipMemcpyAsync(c->d_cd.p, c->img.h_cd.data() + k0, nbc * sizeof(ChainDesc), hipMemcpyHostToDevice, ss));
    HIPCHK(h, hipMemcpyAsync(c->d_start0.p, c->img.h_start0.data() + k0, nbc * sizeof(double), hipMemcpyHostToDevice, ss));
    BatchDev p = chain_only_dev(c, pc, in, h->d_hz.p);
    p.chain_starts = 1;
    p.model_start = 0; /* over tens of thousands of blocks a prediction drifts too far: pass A and the prefix stay */
    p.seg_tiles = p.ntiles;
    p.aux = c->d_aux.p;
    p.start0 = c->d_start0.p;
    p.fix_end = c->fix.end.p;
    p.fix_flag = c->fix.flag.p;
    p.fix_epoch = ++c->fix.epoch;
    p.fix_chunks = (pc.nb + FIXP_WG_ALONE - 1) / FIXP_WG_ALONE;
    p.seed_order = nullptr; /* channel by channel, blocks in order (k_walk) */
    p.seed_lanes = in.nch * ((pc.nb + 63) & ~63);
    HIPCHK(h, walk_chain_launch(ss, p, p.seed_lanes, true, 3, FIXP_WG_ALONE, CarryEvents()));
    HIPCHK(h, hipGetLastError());
    if (want_seeds)
        HIPCHK(h, hipMemcpyAsync(c->img.h_cd.data() + k0, c->d_cd.p, nbc * sizeof(ChainDesc), hipMemcpyDeviceToHost, ss));
    HIPCHK(h, hipStreamSynchronize(ss)); /* the device buffers are the next piece's */
    return GPSBB_OK;
}

/* Every block's start phase from what the lap-parallel pieces brought back: a block starts where the one before ended, or — a
 * channel that was idle or had another prn there — from its own phase */
static void chain_only_lap_seeds(const ChainOnly *c, const PlanIn &in, double *seed)
{
    for (int i = 0; i < in.nch; i++)
        for (int blk = 0; blk < in.nblocks; blk++) {
            const size_t k = (size_t)blk * in.nch + i;
            const ChainDesc &d = c->img.h_cd[k];
            double v = 0.0;
            if (d.prn > 0)
                v = (blk > 0 && c->img.h_cd[k - in.nch].prn == d.prn) ? c->h_lap_end[k - in.nch] : d.carr_phase;
            seed[k] = v;
        }
}

/* ... from what the row-walk pieces brought back */
static void chain_only_walk_seeds(const ChainOnly *c, const PlanIn &in, double *seed)
{
    for (size_t k = 0; k < (size_t)in.nblocks * in.nch; k++)
        seed[k] = c->img.h_cd[k].prn > 0 ? c->img.h_cd[k].carr_phase : 0.0;
}

/* ... and what the call brings back once its last piece is done: the exact phase after the last block, the self-check word */
static int chain_only_finish(gpsbb *h, const ChainOnly *c, const PlanIn &in, double *carr_phase_end)
{
    if (carr_phase_end) {
        ChainCarryDev cc;
        HIPCHK(h, hipMemcpy(&cc, c->d_carry.p, sizeof cc, hipMemcpyDeviceToHost));
        for (int i = 0; i < in.nch; i++)
            carr_phase_end[i] = c->img.h_cd[(size_t)(in.nblocks - 1) * in.nch + i].prn > 0 ? cc.exact_end[i] : 0.0;
    }
    h->last_chain_dev = 1;
    uint32_t st = 0;
    HIPCHK(h, hipMemcpy(&st, c->d_status.p, 4, hipMemcpyDeviceToHost));
    return st ? GPSBB_E_INTERNAL : GPSBB_OK;
}

extern "C" int gpsbb_chain_carrier(gpsbb_t *h, const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp,
                                   double *carr_phase_seed, double *carr_phase_end)
{
    if (!h || !ch || nblocks < 1 || nch < 1 || nch > GPSBB_MAX_CHAN || nsamp < 1 || !(delt > 0.0) || !std::isfinite(delt))
        return GPSBB_E_BADARG;
    if (!h->chain_only && !(h->chain_only = new (std::nothrow) ChainOnly))
        return GPSBB_E_NOMEM;
    ChainOnly *c = h->chain_only;
    const PlanIn in{ch, nblocks, nch, delt, nsamp, GPSBB_CHAIN_CARRIER};
    int rc = plan_chain_only(c->plan, c->img, in, plan_opts(h, NSETS)); /* every error of the arguments, before any HIP call */
    if (rc != GPSBB_OK)
        return rc;
    const bool want_seeds = carr_phase_seed != nullptr;
    rc = chain_only_scratch(h, c, c->plan.laps && want_seeds ? (size_t)nblocks * nch : 0);
    for (size_t k = 0; k < c->plan.pieces.size() && rc == GPSBB_OK; k++)
        rc = (c->plan.laps ? chain_only_lap_piece : chain_only_walk_piece)(h, c, c->plan.pieces[k], in, want_seeds);
    if (rc != GPSBB_OK)
        return rc;
    if (want_seeds)
        (c->plan.laps ? chain_only_lap_seeds : chain_only_walk_seeds)(c, in, carr_phase_seed);
    return chain_only_finish(h, c, in, carr_phase_end);
}

/* what this process holds right now: device buffers, pinned buffers, events (gpsbb_testhooks.h; in both builds) */
extern "C" void gpsbb_test_live(long long out[3])
{
    out[0] = g_live_dev.load(std::memory_order_relaxed);
    out[1] = g_live_pinned.load(std::memory_order_relaxed);
    out[2] = g_live_events.load(std::memory_order_relaxed);
}

#ifdef GPSBB_EXPERIMENTS
/* ---- test hooks (gpsbb_testhooks.h): the shared NCO code, compiled for the host -------------------- */

extern "C" double gpsbb_test_carr_jump(double x, double s, long long n) { return carr_jump(x, s, n); }

extern "C" double gpsbb_test_code_jump(double x, double s, long long n, long long *wraps)
{
    int64_t w = 0;
    double r = code_jump(x, s, n, &w);
    if (wraps)
        *wraps = w;
    return r;
}

namespace {
struct HostSink {
    gpsbb_test_row_t *rows;
    int cap, cnt;
    unsigned long long fetches;
    void row(int32_t n0, uint32_t nav, uint64_t xb, int64_t inc)
    {
        if (cnt < cap) {
            rows[cnt].n0 = n0;
            rows[cnt].nav = nav;
            rows[cnt].xb = xb;
            rows[cnt].inc = inc;
        }
        cnt++;
    }
    void nav_fetch(uint32_t) { fetches++; }
};
} /* namespace */

extern "C" int gpsbb_test_build_rows(int kind, double x0, double s, unsigned nav0, int nsamp,
                                     gpsbb_test_row_t *rows, int cap, double *x_end, unsigned *nav_end)
{
    HostSink sink{rows, cap, 0, 0};
    uint32_t nav = nav0;
    double x = kind == NCO_CODE ? build_rows<NCO_CODE>(x0, s, nav, nsamp, sink)
                                : build_rows<NCO_CARR>(x0, s, nav, nsamp, sink);
    if (x_end)
        *x_end = x;
    if (nav_end)
        *nav_end = nav;
    return sink.cnt;
}

namespace {
struct HostSinkF64 {
    gpsbb_test_row_t *rows;
    int cap, cnt;
    void row(int32_t n0, uint32_t nav, double x, double S, bool after_wrap)
    {
        if (cnt < cap) {
            rows[cnt].n0 = n0;
            rows[cnt].nav = nav | (after_wrap ? 0x40000000u : 0u); /* bit 30: the row follows a wrap */
            rows[cnt].xb = f64_bits(x);
            rows[cnt].inc = (int64_t)f64_bits(S);
        }
        cnt++;
    }
    void nav_fetch(uint32_t) {}
    void table_index_512() {}
};
} /* namespace */

/* the row builder the device pre-pass runs (build_rows_f64): rows as {n0, nav, bits(x), bits(S)} */
extern "C" int gpsbb_test_build_rows_f64(int kind, double x0, double s, unsigned nav0, int nsamp,
                                         gpsbb_test_row_t *rows, int cap, double *x_end, unsigned *nav_end)
{
    HostSinkF64 sink{rows, cap, 0};
    uint32_t nav = nav0;
    double x = kind == NCO_CODE ? build_rows_f64<NCO_CODE>(x0, s, nav, nsamp, sink)
                                : build_rows_f64<NCO_CARR>(x0, s, nav, nsamp, sink);
    if (x_end)
        *x_end = x;
    if (nav_end)
        *nav_end = nav;
    return sink.cnt;
}

/* the host's prediction of a carrier n steps on (CarrDrift: where pass B of the device-side chain starts a segment) */
extern "C" double gpsbb_test_carr_predict(double x0, double s, int n)
{
    const CarrDrift d(s);
    return d.advance(x0, n, s);
}

/* the fixed-point carrier's table index at the first sample of tile t, as the model kernels' pre-pass writes it */
extern "C" double gpsbb_test_fixed_tile_index(uint32_t ph0, int32_t step, int t)
{
    return fixed_tile_index(ph0, step, t);
}

/* The realised error of the model kernels' in-tile models against the reference's own recurrence, over every tile of the
 * batch's LAST run (gpsbb_modelerr.hip.h).  maxima: [GPSBB_MAX_CHAN][GPSBB_TEST_ME_NQ] doubles, counts:
 * [GPSBB_MAX_CHAN][GPSBB_TEST_MEC_NQ]; *which = 1 for k_synth_ev / k_synth_ev_dense / k_synth_ev_fixed, 2 for k_synth_pd. */
extern "C" int gpsbb_test_model_err(gpsbb_batch_t *b, double *maxima, unsigned long long *counts, int *which)
{
    if (!b || !maxima || !counts)
        return GPSBB_E_BADARG;
    gpsbb *h = b->h;
    const BatchPlan &pl = b->plan;
    if (!b->ran || !pl.ev)
        return GPSBB_E_STATE; /* only the model kernels have a model */
    const int rc = gpsbb_sync(h);
    if (rc != GPSBB_OK)
        return rc;
    const BatchDev p = batch_dev(b, b->sets[b->last_set], batch_launch_plan(b));
    DevBuf<double> d_mx;
    DevBuf<unsigned long long> d_cnt;
    const AtExit done{[&] { release_all(d_mx, d_cnt); }};
    const size_t mx_bytes = sizeof(double) * GPSBB_MAX_CHAN * ME_NQ, cnt_bytes = sizeof(unsigned long long) * GPSBB_MAX_CHAN * MEC_NQ;
    HIPCHK(h, (hipError_t)d_mx.reserve((size_t)GPSBB_MAX_CHAN * ME_NQ));
    HIPCHK(h, (hipError_t)d_cnt.reserve((size_t)GPSBB_MAX_CHAN * MEC_NQ));
    HIPCHK(h, hipMemsetAsync(d_mx.p, 0, mx_bytes, h->s_compute));
    HIPCHK(h, hipMemsetAsync(d_cnt.p, 0, cnt_bytes, h->s_compute));
    const size_t threads = (size_t)pl.nblocks * pl.nch * pl.ntiles;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (pl.ev_all_dense)
        hipLaunchKernelGGL(k_model_err_pd, grid, dim3(256), 0, h->s_compute, p, d_mx.p, d_cnt.p);
    else
        hipLaunchKernelGGL(k_model_err_ev, grid, dim3(256), 0, h->s_compute, p, d_mx.p, d_cnt.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->s_compute));
    HIPCHK(h, hipMemcpy(maxima, d_mx.p, mx_bytes, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(counts, d_cnt.p, cnt_bytes, hipMemcpyDeviceToHost));
    if (which)
        *which = pl.ev_all_dense ? 2 : 1;
    return GPSBB_OK;
}

/* What the pre-pass of the batch's LAST run left for the model kernels — the tile states (bit patterns) and data bits (every tile's;
 * for the batches k_synth_ev renders, the tiles that start a granule: below), every end-of-block state — as three 64-bit sums of mixed words: the lap-parallel pre-pass (its reference
 * states on the model or pushed far off it: GPSBB_LAP_JITTER) and the row walks must leave the same bits, whatever the IQ makes of
 * them (tools/table_check.py). */
/* the state granule the batch's tables were built with (BatchDev::st_log2), or a negative error */
extern "C" int gpsbb_test_state_log2(gpsbb_batch_t *b)
{
    return b ? b->plan.st_log2 : GPSBB_E_BADARG;
}
/* ... and the carrier rows' (ev_carr_log2 of it) */
extern "C" int gpsbb_test_state_log2_carr(gpsbb_batch_t *b)
{
    return b ? ev_carr_log2(b->plan.st_log2) : GPSBB_E_BADARG;
}

/* the rule of a granule table's data bits (ev_nav_in_sign, gpsbb_events.hip.h), as the host and the kernels compile it */
extern "C" void gpsbb_test_nav_sign(unsigned long long state_bits, int minus, int g, int e, int used, long long out[6])
{
    const uint64_t stored = ev_nav_in_sign(g) ? ev_state_signed(state_bits, minus != 0) : state_bits;
    const EvNextBitAt nx = ev_next_bit_at(e, used);
    out[0] = (long long)stored;
    out[1] = (long long)ev_state_mag(stored);
    out[2] = (long long)ev_state_bit(stored);
    out[3] = nx.from_end ? 1 : 0;
    out[4] = nx.entry;
    out[5] = ev_nav_in_sign(g) ? 1 : 0;
}

/* plan_batch on its own (no handle, no GPU): the BatchPlan scalars and a 64-bit FNV-1a of every image the plan defines for that
 * batch (0: not one of them), in the order gpsbb_testhooks.h names */
static unsigned long long fnv1a(const void *p, size_t n)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++)
        h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
    return h;
}

template <class T>
static unsigned long long fnv1a(const std::vector<T> &v, bool defined = true)
{
    return defined ? fnv1a(v.data(), v.size() * sizeof(T)) : 0ull;
}

extern "C" int gpsbb_test_plan(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp, unsigned flags, const int opt[5],
                               int carry, const int *carry_prn, double *carry_phase, const int *fixed_prev_prn,
                               const uint32_t *fixed_prev_phase, unsigned long long out[GPSBB_TEST_PLAN_NQ])
{
    if (!opt || !out)
        return GPSBB_E_BADARG;
    static ChainCarryDev none; /* (a carry is present or not: the plan never looks inside) */
    StreamLink lk;
    lk.d_carry = carry ? &none : nullptr;
    lk.carry_prn = carry_prn;
    lk.carry_phase = carry_phase;
    lk.fixed_prev_prn = fixed_prev_prn;
    lk.fixed_prev_phase = fixed_prev_phase;
    BatchPlan pl;
    PlanImages img;
    const int rc = plan_batch(pl, img, PlanIn{ch, nblocks, nch, delt, nsamp, flags}, plan_opts(opt[0], opt[1], opt[2] != 0, opt[3], opt[4]), lk);
    if (rc != GPSBB_OK)
        return rc;
    const bool fixed = (pl.flags & GPSBB_FIXED_CARRIER) != 0, walks = pl.chain_dev && !pl.laps;
    const unsigned long long v[GPSBB_TEST_PLAN_NQ] = {
        (unsigned long long)pl.nblocks, (unsigned long long)pl.nch, (unsigned long long)pl.nsamp, (unsigned long long)pl.ntiles,
        fnv1a(&pl.delt, sizeof pl.delt), pl.flags, pl.ev, pl.ev_dense, pl.ev_all_dense, pl.laps, pl.host_seed,
        (unsigned long long)pl.st_log2, (unsigned long long)pl.nstates, pl.chain_dev, pl.chain_starts, pl.chain_indep, pl.chain_model,
        pl.chain_fix_seq, (unsigned long long)pl.nseg, (unsigned long long)pl.seg_tiles, (unsigned long long)pl.fix_wg,
        (unsigned long long)pl.fix_chunks, (unsigned long long)pl.nsets, pl.total_rows, (unsigned long long)pl.carr_lanes,
        (unsigned long long)pl.chain_lanes, pl.cont0_mask, pl.laps ? fnv1a(pl.lap_chunk0, sizeof pl.lap_chunk0) : 0ull,
        fnv1a(img.h_ch), fnv1a(img.h_evc, pl.ev), fnv1a(img.row_off), fnv1a(img.h_kph0, fixed), fnv1a(img.h_kstep, fixed),
        fnv1a(img.h_cd, walks), fnv1a(img.h_start0, walks), fnv1a(img.h_seed_order), fnv1a(img.h_chain_order, pl.chain_starts),
        carry && carry_phase ? fnv1a(carry_phase, (size_t)pl.nch * sizeof(double)) : 0ull};
    memcpy(out, v, sizeof v);
    return GPSBB_OK;
}

/* plan_launch behind plan_batch: the launch plan's fields in LaunchPlan's order, the number of kernels, then the kernels in order */
extern "C" int gpsbb_test_launch_plan(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp, unsigned flags, const int opt[5],
                                      int carry, const int *carry_prn, double *carry_phase, const int *fixed_prev_prn,
                                      const uint32_t *fixed_prev_phase, int cus, int want_digest, int skip,
                                      long long out[GPSBB_TEST_LAUNCH_NQ])
{
    if (!opt || !out)
        return GPSBB_E_BADARG;
    static ChainCarryDev none;
    StreamLink lk;
    lk.d_carry = carry ? &none : nullptr;
    lk.carry_prn = carry_prn;
    lk.carry_phase = carry_phase;
    lk.fixed_prev_prn = fixed_prev_prn;
    lk.fixed_prev_phase = fixed_prev_phase;
    BatchPlan pl;
    PlanImages img;
    const int rc = plan_batch(pl, img, PlanIn{ch, nblocks, nch, delt, nsamp, flags}, plan_opts(opt[0], opt[1], opt[2] != 0, opt[3], opt[4]), lk);
    if (rc != GPSBB_OK)
        return rc;
    const LaunchPlan lp = plan_launch(pl, LaunchIn{cu_count(cus), want_digest != 0, carry != 0, skip != 0}, launch_opts());
    const std::vector<LaunchRec> ks = launch_list(pl, lp);
    const long long v[GPSBB_TEST_LAUNCH_NF + 1] = {
        lp.prepass, lp.lap_wide, lp.lap_merged, lp.lap_fixed, lp.chain, lp.pass_a, lp.pass_b, lp.fix_wg, lp.carr_lanes, lp.walk_lanes,
        lp.chain_order, lp.seed_ev, lp.seed_lanes, lp.ctr_reset, lp.info_prepass, lp.variant, lp.digest_fused, lp.granule, lp.ev_chunk,
        lp.pd_danger, lp.helpers, lp.grid_x, lp.grid_y, lp.wg, lp.lds, lp.digest_gx, lp.digest_gy, lp.last_kernel, lp.last_chain_dev,
        (long long)ks.size()};
    memset(out, 0, GPSBB_TEST_LAUNCH_NQ * sizeof out[0]);
    memcpy(out, v, sizeof v);
    for (size_t k = 0; k < ks.size() && k < GPSBB_TEST_LAUNCH_KERNELS; k++) {
        const long long r[5] = {ks[k].id, ks[k].gx, ks[k].gy, ks[k].wg, ks[k].lds};
        memcpy(out + GPSBB_TEST_LAUNCH_NF + 1 + 5 * k, r, sizeof r);
    }
    return GPSBB_OK;
}

/* plan_push_side on its own: the side (PUSH_CHAIN_*), and whether the decision took the plan's first step */
extern "C" int gpsbb_test_push_side(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp, unsigned flags, const int opt[5],
                                    int out[2])
{
    if (!ch || !opt || !out || nblocks < 1 || nch < 1 || nch > GPSBB_MAX_CHAN)
        return GPSBB_E_BADARG;
    PushSide side;
    PlanImages img;
    const int rc = plan_push_side(side, img, PlanIn{ch, nblocks, nch, delt, nsamp, flags}, plan_opts(opt[0], opt[1], opt[2] != 0, opt[3], opt[4]));
    out[0] = (int)side.chain;
    out[1] = side.begun;
    return rc;
}

/* plan_chain_only on its own: which pre-pass, the pieces (the first GPSBB_TEST_CHAIN_PLAN_PIECES of them), the images' hashes */
extern "C" int gpsbb_test_chain_plan(const gpsbb_chan_t *ch, int nblocks, int nch, double delt, int nsamp, int seed_where,
                                     unsigned long long out[GPSBB_TEST_CHAIN_PLAN_NQ])
{
    if (!out)
        return GPSBB_E_BADARG;
    ChainOnlyPlan cp;
    PlanImages img;
    const int rc = plan_chain_only(cp, img, PlanIn{ch, nblocks, nch, delt, nsamp, GPSBB_CHAIN_CARRIER}, plan_opts(seed_where, 0, false, 0, NSETS));
    if (rc != GPSBB_OK)
        return rc;
    memset(out, 0, GPSBB_TEST_CHAIN_PLAN_NQ * sizeof out[0]);
    out[0] = cp.laps;
    out[1] = cp.pieces.size();
    out[2] = fnv1a(img.h_cd);
    out[3] = fnv1a(img.h_start0);
    for (size_t k = 0; k < cp.pieces.size() && k < GPSBB_TEST_CHAIN_PLAN_PIECES; k++) {
        const ChainOnlyPiece &pc = cp.pieces[k];
        const unsigned long long v[4] = {(unsigned long long)pc.b0, (unsigned long long)pc.nb, pc.cont0_mask,
                                         cp.laps ? fnv1a(pc.chunk0, sizeof pc.chunk0) : 0ull};
        memcpy(out + 4 + 4 * k, v, sizeof v);
    }
    return GPSBB_OK;
}

extern "C" int gpsbb_test_table_digest(gpsbb_batch_t *b, unsigned long long out[3])
{
    if (!b || !out || !b->ran || !b->plan.ev)
        return GPSBB_E_STATE;
    gpsbb *h = b->h;
    const BatchPlan &pl = b->plan;
    const int rc = gpsbb_sync(h);
    if (rc != GPSBB_OK)
        return rc;
    const BatchDev p = batch_dev(b, b->sets[b->last_set], batch_launch_plan(b));
    auto mix = [](unsigned long long z) { z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29; return z; };
    const int nst = pl.nstates;
    const size_t nx = (size_t)pl.nblocks * 2 * pl.nch * (size_t)nst, nn = (size_t)pl.nblocks * pl.nch * (size_t)nst, ne = (size_t)pl.nblocks * pl.nch;
    /* The states keyed by the tile t they start: every tile's, but for a batch that k_synth_ev renders — whose tables hold one state
     * per granule behind the lap-parallel pre-pass (BatchDev::st_log2) and one per tile behind the row walks — those of the tiles that
     * start a granule of the size the lap-parallel pre-pass would use: the two pre-passes' tables digest alike where they agree, and
     * every other batch's are compared tile by tile.  The granule is per kind: a carrier row's is ev_carr_log2 of the code's, in the
     * tables and in the key alike */
    const int dg = pl.ev_dense || (pl.flags & GPSBB_FIXED_CARRIER) ? 0 : (int)GPSBB_KNOB_LONG("GPSBB_EV_STATE_LOG2", GPSBB_EV_STATE_LOG2);
    const int kg = dg > pl.st_log2 ? dg : pl.st_log2; /* the key's granule (the code's) */
    std::vector<unsigned long long> hx(nx);
    std::vector<uint32_t> hn(nn);
    std::vector<gpsbb_chan_state_t> he(ne);
    HIPCHK(h, hipMemcpy(hx.data(), p.tile_x, nx * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(hn.data(), p.tile_nav, nn * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(he.data(), p.end, ne * sizeof(gpsbb_chan_state_t), hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = 0;
    /* (idle channels' entries are whatever the allocation held: only active block-channels count) */
    std::vector<gpsbb_chan_t> hc(ne);
    HIPCHK(h, hipMemcpy(hc.data(), p.ch, ne * sizeof(gpsbb_chan_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < ne; k++) {
        if (hc[k].prn <= 0)
            continue;
        const size_t blk = k / (size_t)pl.nch, i = k % (size_t)pl.nch;
        if (ev_nav_in_sign(pl.st_log2)) {
            /* A granule table has no tile_nav words: its code states carry the data bit in force in their signs (ev_nav_in_sign).
             * The states and the words every other table holds, from them: bit 0 is the sign; bit 1 — the bit in force after the
             * next roll-over — is the bit in force behind the first roll-over from the entry on (a state below the one before it:
             * a granule advances by less than a period), and past the block's last one what the end state's counters say */
            unsigned long long *x = &hx[ev_tile_x_row(blk, pl.nch, (int)i, NCO_CODE, nst)];
            uint32_t *nv = &hn[ev_tile_nav_row(blk, pl.nch, (int)i, nst)];
            const uint32_t nav_end = nav_pack(he[k].icode, he[k].ibit, he[k].iword);
            uint32_t after = nav_bit(hc[k].dwrd, nav_advance(nav_end)) < 0 ? 1u : 0u;
            /* (what follows the row's last entry is the block's end state: ev_next_bit_at) */
            uint32_t next_bit = he[k].dataBit < 0 ? 1u : 0u;
            unsigned long long next_mag;
            memcpy(&next_mag, &he[k].code_phase, 8);
            for (int e = nst - 1; e >= 0; e--) {
                const uint32_t here = ev_state_bit(x[e]);
                x[e] = ev_state_mag(x[e]);
                if (next_mag < x[e]) /* (non-negative doubles compare as their bits do) */
                    after = next_bit;
                nv[e] = here | (after << 1);
                next_bit = here;
                next_mag = x[e];
            }
        }
        for (int kind = 0; kind < 2; kind++)
            for (int t = 0; t < pl.ntiles; t += 1 << ev_kind_log2(kg, kind)) {
                const size_t at = ev_tile_x_row(blk, pl.nch, (int)i, kind, pl.ntiles) + t;
                out[0] += mix(hx[ev_tile_x_row(blk, pl.nch, (int)i, kind, nst) + ev_state_at(pl.st_log2, kind, t).entry] +
                              0x9E3779B97F4A7C15ull * (at + 1));
            }
        for (int t = 0; t < pl.ntiles; t += 1 << kg) {
            const size_t at = ev_tile_nav_row(blk, pl.nch, (int)i, pl.ntiles) + t;
            out[1] += mix((unsigned long long)(hn[ev_tile_nav_row(blk, pl.nch, (int)i, nst) + ev_state_at(pl.st_log2, NCO_CODE, t).entry] & 3u) +
                          0x9E3779B97F4A7C15ull * (at + 1));
        }
        unsigned long long w[5];
        memcpy(w, &he[k], sizeof w);
        for (int q = 0; q < 4; q++) /* carr_phase, code_phase, (iword, ibit), (icode, dataBit); codeCA with the padding */
            out[2] += mix(w[q] + 0x9E3779B97F4A7C15ull * (k * 5 + q + 1));
        out[2] += mix((unsigned long long)(uint32_t)he[k].codeCA + 0x9E3779B97F4A7C15ull * (k * 5 + 5));
    }
    return GPSBB_OK;
}

/* the derived budgets this build was compiled with, in units of 2^-32: EV_MODEL_ERR, EV_T_EPS, PD_BAND */
extern "C" void gpsbb_test_budgets(double out[3])
{
    out[0] = EV_MODEL_ERR * 0x1p+32;
    out[1] = EV_T_EPS * 0x1p+32;
    out[2] = (double)PD_BAND;
}

extern "C" unsigned long long gpsbb_test_row_bound(int kind, double s_abs, int nsamp)
{
    return kind == NCO_CODE ? row_bound(s_abs, 1023.0, 9, nsamp) : row_bound(s_abs, 1.0, -1, nsamp);
}

/* FETCH_SIZE calibration: `bytes` bytes of d_src (device memory, at least that big) read once with the tile states' pattern
 * (k_read_pattern: 32 rows of 2442 doubles per wavefront, what a wavefront of k_synth_ev reads of one block); returns the bytes
 * actually read */
extern "C" long long gpsbb_test_read_pattern(gpsbb_t *h, const void *d_src, size_t bytes)
{
    if (!h || !d_src)
        return GPSBB_E_BADARG;
    const int rows = 32, cols = 2442;
    const size_t per_wave = (size_t)rows * cols * 8;
    size_t waves = bytes / per_wave;
    waves -= waves % 4;
    if (waves < 4)
        return GPSBB_E_BADARG;
    DevBuf<double> d_sink;
    if (d_sink.reserve(1) != hipSuccess)
        return GPSBB_E_NOMEM;
    hipLaunchKernelGGL(k_read_pattern, dim3((unsigned)(waves / 4)), dim3(256), 0, h->s_compute, (const double *)d_src, rows, cols, d_sink.p);
    const hipError_t e = hipStreamSynchronize(h->s_compute);
    d_sink.release();
    return e == hipSuccess ? (long long)(waves * per_wave) : (long long)GPSBB_E_HIP;
}

extern "C" unsigned long long gpsbb_test_despread_exact(gpsbb_batch *b) { return b ? b->ds_last_exact : 0ull; }
extern "C" float gpsbb_test_despread_ms(gpsbb_batch *b) { return b ? b->ds_tm.ms() : -1.0f; }
extern "C" float gpsbb_test_acquire_ms(gpsbb *h) { return h ? h->acq_tm.ms() : -1.0f; }
extern "C" float gpsbb_test_track_ms(gpsbb *h) { return h ? h->trk_tm.ms() : -1.0f; }
extern "C" float gpsbb_test_fir_ms(gpsbb *h) { return h ? h->fir_tm.ms() : -1.0f; }

extern "C" int gpsbb_test_fir_tile(void) { return FIR_TILE; }
extern "C" float gpsbb_test_psd_ms(gpsbb *h) { return h ? h->psd_tm.ms() : -1.0f; }
extern "C" int gpsbb_test_psd_run(int log2n) { return log2n < PSD_MIN_LOG2N || log2n > PSD_MAX_LOG2N ? -1 : psd_min_run(log2n); }
extern "C" float gpsbb_test_exc_ms(gpsbb *h) { return h ? h->exc_tm.ms() : -1.0f; }
extern "C" int gpsbb_test_exc_run(int log2n) { return log2n < EXC_MIN_LOG2N || log2n > EXC_MAX_LOG2N ? -1 : exc_min_run(log2n); }
extern "C" int gpsbb_test_exc_host(const gpsbb_exc_t *e, const int16_t *w, long nsamp, const int16_t *hist_in, int16_t *out, int16_t *hist_out,
                                   uint64_t *clipped, uint64_t *excised, int64_t *peak)
{
    if (!e || e->log2n < EXC_MIN_LOG2N || e->log2n > EXC_MAX_LOG2N)
        return GPSBB_E_BADARG;
    std::vector<psd_c> work((size_t)1 << e->log2n), half((size_t)1 << (e->log2n - 1), psd_c{0, 0});
    return exc_host(e, w, nsamp, hist_in, psd_table(), psd_table() + PSD_TW, work.data(), half.data(), out, hist_out, clipped, excised, peak)
               ? GPSBB_OK
               : GPSBB_E_BADARG;
}
extern "C" float gpsbb_test_blank_ms(gpsbb *h) { return h ? h->blank_tm.ms() : -1.0f; }
extern "C" void gpsbb_test_blank_nt(int on) { g_blank_nt = on != 0; }
extern "C" int gpsbb_test_blank_tile(int *run)
{
    if (run)
        *run = BLANK_MIN_RUN;
    return BLANK_TILE;
}
extern "C" int gpsbb_test_blank_host(const gpsbb_blank_t *b, const int16_t *w, long nsamp, const int16_t *hist_in, int16_t *out, int16_t *hist_out,
                                     uint64_t *blanked, uint64_t *triggers)
{
    return blank_host(b, w, nsamp, hist_in, out, hist_out, blanked, triggers) ? GPSBB_OK : GPSBB_E_BADARG;
}

#ifdef GPSBB_WG_TRACE
/* The workgroup trace of the measurement build (gpsbb_kernels.hip.h: wg_trace_leave; make trace; tools/corun_diag.py).
 * _begin: (re)arm the trace with room for `cap` records; _read: wait for the device, copy out up to `cap` records of
 * WG_TRACE_WORDS 64-bit words, return how many were written (the device counts on past the capacity). */
namespace {
DevBuf<unsigned long long> g_trace_buf;
unsigned g_trace_cap = 0; /* records */
}
extern "C" int gpsbb_test_wg_trace_begin(unsigned cap)
{
    if (hipDeviceSynchronize() != hipSuccess)
        return GPSBB_E_HIP;
    if (cap > g_trace_cap) {
        g_trace_cap = 0;
        g_trace_buf.release(); /* (exactly what is asked, as ever: an empty DevBuf takes no head-room) */
        if (g_trace_buf.reserve((size_t)cap * WG_TRACE_WORDS) != hipSuccess)
            return GPSBB_E_NOMEM;
        g_trace_cap = cap;
    }
    const unsigned zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_wg_trace), &g_trace_buf.p, sizeof g_trace_buf.p) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_wg_trace_cap), &cap, sizeof cap) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_wg_trace_n), &zero, sizeof zero) != hipSuccess)
        return GPSBB_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? GPSBB_OK : GPSBB_E_HIP;
}
extern "C" long gpsbb_test_wg_trace_read(unsigned long long *out, unsigned cap)
{
    if (hipDeviceSynchronize() != hipSuccess)
        return GPSBB_E_HIP;
    unsigned n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_wg_trace_n), sizeof n) != hipSuccess)
        return GPSBB_E_HIP;
    const unsigned have = n < g_trace_cap ? n : g_trace_cap, take = have < cap ? have : cap;
    if (take && hipMemcpy(out, g_trace_buf.p, (size_t)take * WG_TRACE_WORDS * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return GPSBB_E_HIP;
    return (long)n;
}
#endif
#endif /* GPSBB_EXPERIMENTS */
