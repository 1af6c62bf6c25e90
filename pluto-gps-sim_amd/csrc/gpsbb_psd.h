/*
 * gpsbb_psd.h — the rules of the power spectrum (include/gpsbb.h, gpsbb_device_psd: the definition in full) that do not need a
 * GPU: what a gpsbb_psd_t may hold, the segment count, the overflow bound and the smallest shift, the windows, the twiddle table
 * (one octant computed, the rest reflected), the load, the twiddle product and the butterfly of one radix-2 step, and the whole
 * definition in plain C over view samples in host memory.  Plain C++: k_psd loads, multiplies and adds with psd_load, psd_tmul and
 * psd_bfly as they stand here, gpsbb.hip's entry points call the rest, tools/psd_asan.cpp runs all of it under the host sanitizers.
 */
#ifndef GPSBB_PSD_H
#define GPSBB_PSD_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gpsbb.h"

#if defined(__HIPCC__)
#define GPSBB_PSD_HD __host__ __device__ inline
#else
#define GPSBB_PSD_HD inline
#endif

namespace gpsbb_impl {

constexpr int PSD_MIN_LOG2N = 6, PSD_MAX_LOG2N = 12, PSD_MAX_SHIFT = 30, PSD_TW = 2048;
constexpr long PSD_MAX_HOP = 1L << 20, PSD_MAX_NSEG = 1L << 20;
static_assert((1 << PSD_MAX_LOG2N) == GPSBB_PSD_MAX_N && PSD_TW * 2 == GPSBB_PSD_MAX_N, "one table for every N");

struct alignas(8) psd_c {
    int32_t re, im;
};

/* Wbits of a view (acq_view_format's number): |w| <= 2^Wbits */
GPSBB_PSD_HD int psd_wbits(int fmt) { return fmt == 0 ? 15 : (fmt == 1 ? 7 : 0); }

/* x of the definition for one component: (w * win * 2^(15 - Wbits)) >> 1 with wmul = 2^(15 - Wbits); |w * win * wmul| <= 2^30 */
GPSBB_PSD_HD int32_t psd_load(int32_t w, int32_t win, int32_t wmul) { return (w * win * wmul) >> 1; }

/* t = v * (c - i s) of the definition: products and sums in int64, rounded to nearest, halves up */
GPSBB_PSD_HD psd_c psd_tmul(psd_c v, int32_t c, int32_t s)
{
    const int64_t re = (int64_t)v.re * c + (int64_t)v.im * s + ((int64_t)1 << 29);
    const int64_t im = (int64_t)v.im * c - (int64_t)v.re * s + ((int64_t)1 << 29);
    return psd_c{(int32_t)(re >> 30), (int32_t)(im >> 30)};
}

/* u, v <- (u + t + 1) >> 1, (u - t + 1) >> 1: |u|, |t| < 2^30.3, so the sums stay inside int32 (include/gpsbb.h) */
GPSBB_PSD_HD void psd_bfly(psd_c &u, psd_c &v, psd_c t)
{
    const psd_c p{(u.re + t.re + 1) >> 1, (u.im + t.im + 1) >> 1};
    v = psd_c{(u.re - t.re + 1) >> 1, (u.im - t.im + 1) >> 1};
    u = p;
}

/* one bin's term of the power sum */
GPSBB_PSD_HD uint64_t psd_power(psd_c X, int shift)
{
    const int64_t a = X.re >> shift, b = X.im >> shift;
    return (uint64_t)(a * a) + (uint64_t)(b * b);
}

/* nseg of the definition; 0: nsamp < N, or arguments outside their ranges */
inline long psd_nseg(int log2n, long hop, long nsamp)
{
    if (log2n < PSD_MIN_LOG2N || log2n > PSD_MAX_LOG2N || hop < 1 || hop > PSD_MAX_HOP || nsamp < (1L << log2n))
        return 0;
    return (nsamp - (1L << log2n)) / hop + 1;
}

/* nseg * 2 * ((B >> shift) + 1)^2 < 2^64 with B = 2^30 */
inline bool psd_fits(long nseg, int shift)
{
    if (nseg < 1 || nseg > PSD_MAX_NSEG || shift < 0 || shift > PSD_MAX_SHIFT)
        return false;
    const unsigned __int128 t = (((unsigned __int128)1 << 30) >> shift) + 1;
    return (unsigned __int128)(uint64_t)nseg * 2u * t * t < ((unsigned __int128)1 << 64);
}

inline int psd_min_shift(long nseg)
{
    for (int s = 0; s <= PSD_MAX_SHIFT; s++)
        if (psd_fits(nseg, s))
            return s;
    return GPSBB_E_BADARG; /* nseg outside [1, 2^20]: shift 30 fits every legal count */
}

/* every field in range, the samples there, the bound kept; *nseg: the segments */
inline bool psd_ok(const gpsbb_psd_t *p, long nsamp, long *nseg)
{
    if (!p || p->shift < 0 || p->shift > PSD_MAX_SHIFT)
        return false;
    const long n = psd_nseg(p->log2n, (long)p->hop, nsamp);
    if (n < 1 || n > PSD_MAX_NSEG || !psd_fits(n, p->shift))
        return false;
    if (nseg)
        *nseg = n;
    return true;
}

/* c[k] = nearbyint(2^30 cos(2 pi k / 4096)), s[k] likewise with sin, k in [0, 2048): the first octant computed, the second its
 * mirror image (cos and sin change places), the second quadrant the first reflected — every symmetry holds by construction */
inline void psd_twiddles(int32_t c[PSD_TW], int32_t s[PSD_TW])
{
    const double w = 2.0 * 3.14159265358979323846 / 4096.0;
    for (int k = 0; k <= 512; k++) {
        c[k] = (int32_t)nearbyint(ldexp(cos(w * (double)k), 30));
        s[k] = (int32_t)nearbyint(ldexp(sin(w * (double)k), 30));
    }
    s[512] = c[512];
    for (int k = 513; k <= 1024; k++) {
        c[k] = s[1024 - k];
        s[k] = c[1024 - k];
    }
    for (int k = 1025; k < PSD_TW; k++) {
        c[k] = -c[2048 - k];
        s[k] = s[2048 - k];
    }
}

/* the 11-bit reversal of x: k_psd keeps the table in this order (gpsbb_psd.hip.h) */
inline uint32_t psd_brev11(uint32_t x)
{
    uint32_t r = 0;
    for (int b = 0; b < 11; b++)
        r |= ((x >> b) & 1u) << (10 - b);
    return r;
}

inline int psd_make(gpsbb_psd_t *p, int log2n, long hop, int window, long nsamp)
{
    if (!p || log2n < PSD_MIN_LOG2N || log2n > PSD_MAX_LOG2N || hop > PSD_MAX_HOP || (window != 0 && window != 1))
        return GPSBB_E_BADARG;
    const int N = 1 << log2n;
    if (hop <= 0)
        hop = window ? N / 2 : N;
    const long nseg = psd_nseg(log2n, hop, nsamp);
    if (nseg < 1 || nseg > PSD_MAX_NSEG)
        return GPSBB_E_BADARG;
    gpsbb_psd_t o;
    memset(&o, 0, sizeof o);
    o.log2n = log2n;
    o.hop = (int32_t)hop;
    o.shift = psd_min_shift(nseg);
    if (window == 0) {
        for (int n = 0; n < N; n++)
            o.win[n] = 16384;
    } else { /* Hann, periodic: win[0] = 0, win[N / 2] = 16384, win[N - n] = win[n] by reflection */
        const double w = 2.0 * 3.14159265358979323846 / (double)N;
        for (int n = 0; n <= N / 2; n++)
            o.win[n] = (int16_t)nearbyint(16384.0 * 0.5 * (1.0 - cos(w * (double)n)));
        for (int n = N / 2 + 1; n < N; n++)
            o.win[n] = o.win[N - n];
    }
    *p = o;
    return GPSBB_OK;
}

/* 4^shift * N * 4^(Wbits - 14) / (nseg * sum of win^2); NAN: arguments the call refuses, or a window of zeros */
inline double psd_scale(const gpsbb_psd_t *p, long nseg, int fmt)
{
    if (!p || fmt < 0 || fmt > 2 || p->log2n < PSD_MIN_LOG2N || p->log2n > PSD_MAX_LOG2N || p->shift < 0 || p->shift > PSD_MAX_SHIFT || nseg < 1)
        return NAN;
    const int N = 1 << p->log2n;
    double sw = 0.0;
    for (int n = 0; n < N; n++)
        sw += (double)p->win[n] * (double)p->win[n];
    if (!(sw > 0.0))
        return NAN;
    return ldexp((double)N, 2 * p->shift + 2 * (psd_wbits(fmt) - 14)) / ((double)nseg * sw);
}

/* The definition in plain C over view samples w [nsamp][2] in host memory (already impaired and quantised; fmt names the view):
 * psd [N] in natural bin order.  work: [2 * N] psd_c.  The reference the sanitizer run checks; false: arguments the call refuses */
inline bool psd_host(const gpsbb_psd_t *p, const int16_t *w, long nsamp, int fmt, const int32_t *c, const int32_t *s, psd_c *work, uint64_t *psd,
                     long *nseg_out)
{
    long nseg = 0;
    if (!psd_ok(p, nsamp, &nseg) || !w || !psd || !work || fmt < 0 || fmt > 2)
        return false;
    const int L = p->log2n, N = 1 << L;
    const int32_t wmul = 1 << (15 - psd_wbits(fmt));
    for (int k = 0; k < N; k++)
        psd[k] = 0;
    for (long sg = 0; sg < nseg; sg++) {
        const int16_t *x = w + 2 * sg * (long)p->hop;
        for (int n = 0; n < N; n++) {
            uint32_t r = 0;
            for (int b = 0; b < L; b++)
                r |= (((uint32_t)n >> b) & 1u) << (L - 1 - b);
            work[r] = psd_c{psd_load(x[2 * n], p->win[n], wmul), psd_load(x[2 * n + 1], p->win[n], wmul)};
        }
        for (int m = 2; m <= N; m <<= 1) {
            const int h = m / 2;
            for (int j0 = 0; j0 < N; j0 += m)
                for (int j = 0; j < h; j++) {
                    const int k = j * (4096 / m);
                    psd_bfly(work[j0 + j], work[j0 + j + h], psd_tmul(work[j0 + j + h], c[k], s[k]));
                }
        }
        for (int k = 0; k < N; k++)
            psd[k] += psd_power(work[k], p->shift);
    }
    if (nseg_out)
        *nseg_out = nseg;
    return true;
}

} /* namespace gpsbb_impl */
#endif
