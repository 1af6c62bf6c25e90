/*
 * gpsbb_blank.h — the rules of the pulse blanker (include/gpsbb.h, gpsbb_device_blank: the definition in full) that do not need a
 * GPU: what a gpsbb_blank_t may hold, a sample's power, the two host functions that make a plan, the launch geometry, and the whole
 * definition in plain C over view samples in host memory.  Plain C++: k_blank squares with blank_pow and is launched by
 * blank_geometry as they stand here, gpsbb.hip's entry points call the rest, tools/blank_asan.cpp runs all of it under the host
 * sanitizers.
 */
#ifndef GPSBB_BLANK_H
#define GPSBB_BLANK_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gpsbb.h"

#if defined(__HIPCC__)
#define GPSBB_BLANK_HD __host__ __device__ inline
#else
#define GPSBB_BLANK_HD inline
#endif

namespace gpsbb_impl {

constexpr int BLANK_WG = 256;
constexpr int BLANK_TILE = 4096;     /* outputs of a tile */
constexpr int BLANK_MIN_RUN = 2;     /* tiles a workgroup takes, one after the other, at least ... */
constexpr int BLANK_MAX_WGS = 16384; /* ... and more where the grid would pass this many workgroups */
constexpr int BLANK_RCP_BITS = 20;   /* q / R = (q * ceil(2^20 / R)) >> 20 for q < 2^13, R < 128 */
static_assert(GPSBB_BLANK_MAX_HIST == 1341 && sizeof(gpsbb_blank_t) == 24, "gpsbb_blank_t layout");

/* a plan the call serves */
inline bool blank_ok(const gpsbb_blank_t *b)
{
    return b && b->win >= 1 && b->win <= GPSBB_BLANK_MAX_WIN && b->pre >= 0 && b->pre <= GPSBB_BLANK_MAX_PRE && b->hold >= 0 &&
           b->hold <= GPSBB_BLANK_MAX_HOLD && b->_pad == 0;
}

/* K of the definition: the samples before a call's first that its outputs depend on */
inline int blank_hist(const gpsbb_blank_t *b) { return b->pre + b->hold + b->win - 1; }

/* p of the definition from a sample as it lies in memory (Q << 16 | I): at most 2^31, so it fits 32 bits */
GPSBB_BLANK_HD uint32_t blank_pow(uint32_t w)
{
    const int32_t i = (int32_t)(w << 16) >> 16, q = (int32_t)w >> 16;
    return (uint32_t)(i * i) + (uint32_t)(q * q);
}

/* The trigger bits of a tile, G + hold + at most BLANK_TILE of them, are shared out R consecutive ones per lane.  R is odd: lanes
 * that walk their shares in step are then R dwords apart in LDS, and an odd stride visits every bank of (a / 4) mod 32 once per
 * 32 lanes.  At most 21. */
inline int blank_share(int G, int hold) { return ((BLANK_TILE + G + hold + BLANK_WG - 1) / BLANK_WG) | 1; }

/* the run (tiles per workgroup) and the grid for nsamp samples */
inline void blank_geometry(long nsamp, long *run, long *nwg)
{
    const long tiles = (nsamp + BLANK_TILE - 1) / BLANK_TILE;
    long r = (tiles + BLANK_MAX_WGS - 1) / BLANK_MAX_WGS;
    r = r < BLANK_MIN_RUN ? BLANK_MIN_RUN : r;
    *run = r;
    *nwg = (tiles + r - 1) / r;
}

/* thr as a double to the plan: false where it does not fit */
inline bool blank_thr(double t, uint64_t *thr)
{
    t = floor(t);
    if (!std::isfinite(t) || t < 0.0 || !(t < 0x1p+64))
        return false;
    *thr = (uint64_t)t;
    return true;
}

inline int blank_make(gpsbb_blank_t *b, int win, int pre, int hold, double floor_ms, double thr_db)
{
    if (!b || !std::isfinite(floor_ms) || !std::isfinite(thr_db) || floor_ms < 0.0)
        return GPSBB_E_BADARG;
    gpsbb_blank_t o;
    memset(&o, 0, sizeof o);
    o.win = win <= 0 ? 8 : win;
    if (o.win > GPSBB_BLANK_MAX_WIN)
        return GPSBB_E_BADARG;
    o.pre = pre < 0 ? o.win : pre;
    o.hold = hold < 0 ? o.win : hold;
    if (!blank_ok(&o) || !blank_thr(pow(10.0, (thr_db <= 0.0 ? 6.0 : thr_db) / 10.0) * floor_ms * (double)o.win, &o.thr))
        return GPSBB_E_BADARG;
    *b = o;
    return GPSBB_OK;
}

/* thr alone, from the lower median of short blocks' sums of squares; b is changed only where GPSBB_OK */
inline int blank_from_level(gpsbb_blank_t *b, const gpsbb_level_t *lv, long n, int shift, double thr_db)
{
    if (!b || !lv || n < 1 || shift < 0 || shift > 7 || !std::isfinite(thr_db) || b->win < 1 || b->win > GPSBB_BLANK_MAX_WIN || b->pre < 0 ||
        b->pre > GPSBB_BLANK_MAX_PRE || b->hold < 0 || b->hold > GPSBB_BLANK_MAX_HOLD || lv[0].n == 0)
        return GPSBB_E_BADARG;
    std::vector<double> v((size_t)n);
    for (long k = 0; k < n; k++) {
        if (lv[k].n != lv[0].n)
            return GPSBB_E_BADARG;
        v[(size_t)k] = (double)lv[k].sumsq[0] + (double)lv[k].sumsq[1]; /* exact below 2^53: blocks are short */
    }
    std::nth_element(v.begin(), v.begin() + (n - 1) / 2, v.end());
    const double med = v[(size_t)((n - 1) / 2)];
    uint64_t thr = 0;
    if (!blank_thr(pow(10.0, thr_db / 10.0) * med * (double)b->win / ((double)lv[0].n * (double)(1 << (2 * shift))), &thr))
        return GPSBB_E_BADARG;
    b->thr = thr;
    return GPSBB_OK;
}

/* The definition in plain C over view samples w [nsamp][2] in host memory (already impaired): out [nsamp][2], hist_out [K][2] (may
 * be hist_in).  hist_in: [K][2] or NULL (zeros).  false: arguments the call refuses */
inline bool blank_host(const gpsbb_blank_t *b, const int16_t *w, long nsamp, const int16_t *hist_in, int16_t *out, int16_t *hist_out,
                       uint64_t *blanked, uint64_t *triggers)
{
    if (!blank_ok(b) || !w || !out || nsamp < 1)
        return false;
    const long L = b->win, G = b->pre, D = b->pre + b->hold, K = blank_hist(b);
    /* component c of w[n], n in [-K, nsamp) */
    auto at = [&](long n, int c) -> int32_t { return n >= 0 ? w[2 * n + c] : (hist_in ? hist_in[2 * (n + K) + c] : 0); };
    uint64_t nb = 0, nt = 0;
    long last = -D - 1 - K; /* the latest j <= m with trig[j]; none yet */
    for (long j = -D; j < nsamp; j++) {
        uint64_t s = 0;
        for (long k = 0; k < L; k++) { /* j - k >= -D - (L - 1) = -K */
            const int64_t i = at(j - k, 0), q = at(j - k, 1);
            s += (uint64_t)(i * i) + (uint64_t)(q * q);
        }
        if (s > b->thr) {
            last = j;
            nt += j >= 0;
        }
        if (j >= 0) { /* out[m] at m = j: every trig[j'] with j' <= m is known */
            const bool z = last >= j - D;
            nb += z;
            out[2 * j] = z ? 0 : (int16_t)at(j - G, 0);
            out[2 * j + 1] = z ? 0 : (int16_t)at(j - G, 1);
        }
    }
    if (hist_out && K > 0) {
        if (nsamp >= K)
            memcpy(hist_out, w + 2 * (nsamp - K), (size_t)K * 4);
        else {
            if (hist_in)
                memmove(hist_out, hist_in + 2 * nsamp, (size_t)(K - nsamp) * 4);
            else
                memset(hist_out, 0, (size_t)(K - nsamp) * 4);
            memcpy(hist_out + 2 * (K - nsamp), w, (size_t)nsamp * 4);
        }
    }
    if (blanked)
        *blanked = nb;
    if (triggers)
        *triggers = nt;
    return true;
}

} /* namespace gpsbb_impl */
#endif
