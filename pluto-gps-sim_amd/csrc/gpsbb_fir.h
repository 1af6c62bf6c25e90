/*
 * gpsbb_fir.h — the rules of the front-end filter (include/gpsbb.h, gpsbb_device_fir: the definition in full) that do not need a
 * GPU: what a gpsbb_fir_t may hold, the rounding and the clamp of one output component, the taps from a cutoff and an attenuation
 * (a Kaiser-windowed sinc), and the filter itself in plain C over samples in host memory.  Plain C++: k_fir rounds and clamps
 * with fir_round and fir_clamp as they stand here, gpsbb.hip's entry points call the rest, tools/fir_asan.cpp runs all of it
 * under the host sanitizers.
 */
#ifndef GPSBB_FIR_H
#define GPSBB_FIR_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gpsbb.h"

#if defined(__HIPCC__)
#define GPSBB_FIR_HD __host__ __device__ inline
#else
#define GPSBB_FIR_HD inline
#endif

namespace gpsbb_impl {

constexpr int FIR_MAX_DECIM = 16, FIR_MAX_SHIFT = 16, FIR_MAX_SUM = 65535;

/* y of the definition: acc for shift 0, else (acc + (1 << (shift - 1))) >> shift with an arithmetic shift, written as the floor
 * plus the bit below it: acc + 2^15 can reach 2^31 (every tap negative, every sample -32768), the two terms here cannot */
GPSBB_FIR_HD int32_t fir_round(int32_t acc, int shift) { return shift ? (acc >> shift) + ((acc >> (shift - 1)) & 1) : acc; }
GPSBB_FIR_HD int32_t fir_clamp(int32_t y) { return y < -32768 ? -32768 : (y > 32767 ? 32767 : y); }

inline bool fir_ok(const gpsbb_fir_t *f)
{
    if (!f || f->ntaps < 1 || f->ntaps > GPSBB_FIR_MAX_TAPS || f->decim < 1 || f->decim > FIR_MAX_DECIM || f->shift < 0 ||
        f->shift > FIR_MAX_SHIFT)
        return false;
    int32_t sum = 0;
    for (int k = 0; k < f->ntaps; k++)
        sum += f->h[k] < 0 ? -(int32_t)f->h[k] : (int32_t)f->h[k]; /* at most 129 * 32768 */
    return sum <= FIR_MAX_SUM;
}

/* I0(x), the modified Bessel function of order zero, as its power series: sum over m of ((x / 2)^m / m!)^2.  The terms fall
 * once m > x / 2; beta stays below 20 here (fir_make), so 64 terms are far more than a double holds */
inline double fir_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int m = 1; m < 64; m++) {
        term *= q / ((double)m * (double)m);
        sum += term;
        if (term < sum * 1e-18)
            break;
    }
    return sum;
}

/* Kaiser's beta for a stopband atten_db down */
inline double fir_beta(double a)
{
    if (a > 50.0)
        return 0.1102 * (a - 8.7);
    if (a >= 21.0)
        return 0.5842 * pow(a - 21.0, 0.4) + 0.07886 * (a - 21.0);
    return 0.0;
}

inline int fir_make(gpsbb_fir_t *f, int ntaps, int decim, double cutoff, double atten_db)
{
    if (!f || ntaps < 1 || ntaps > GPSBB_FIR_MAX_TAPS || decim < 1 || decim > FIR_MAX_DECIM || !isfinite(cutoff) || !isfinite(atten_db))
        return GPSBB_E_BADARG;
    if (!(cutoff > 0.0)) cutoff = 0.8;
    if (!(atten_db > 0.0)) atten_db = 60.0;
    if (cutoff > 1.0 || atten_db > 180.0) /* (beta below 20: fir_i0's series) */
        return GPSBB_E_BADARG;
    const double fc = cutoff * 0.5 / (double)decim, beta = fir_beta(atten_db), mid = 0.5 * (double)(ntaps - 1);
    const double pi = 3.141592653589793, i0b = fir_i0(beta);
    double g[GPSBB_FIR_MAX_TAPS], sum = 0.0;
    for (int k = 0; k < ntaps; k++) {
        const double t = (double)k - mid, x = 2.0 * fc * t;
        const double sinc = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
        const double r = mid > 0.0 ? t / mid : 0.0, in = 1.0 - r * r;
        g[k] = 2.0 * fc * sinc * fir_i0(beta * sqrt(in > 0.0 ? in : 0.0)) / i0b;
        sum += g[k];
    }
    if (!isfinite(sum) || !(fabs(sum) > 1e-9))
        return GPSBB_E_BADARG;
    gpsbb_fir_t o;
    memset(&o, 0, sizeof o);
    o.ntaps = ntaps;
    o.decim = decim;
    for (o.shift = 15; o.shift >= 14; o.shift--) {
        bool fits = true;
        int64_t total = 0;
        for (int k = 0; k < ntaps; k++) {
            const double v = nearbyint(g[k] / sum * (double)(1 << o.shift));
            fits = fits && fabs(v) <= 32767.0;
            total += fits ? (int64_t)v : 0;
            o.h[k] = fits ? (int16_t)v : 0;
        }
        if (!fits)
            continue;
        const int64_t c = (int64_t)o.h[(ntaps - 1) / 2] + ((int64_t)1 << o.shift) - total; /* the DC gain exactly one */
        if (c > 32767 || c < -32768)
            continue;
        o.h[(ntaps - 1) / 2] = (int16_t)c;
        break;
    }
    if (o.shift < 14 || !fir_ok(&o))
        return GPSBB_E_BADARG;
    *f = o;
    return GPSBB_OK;
}

/* The definition in plain C over view samples w [nsamp][2] in host memory (already impaired): y [nsamp / D][2], the history handed
 * on and the clip count; hist_in and hist_out as gpsbb_device_fir's (either may be NULL, they may be the same).  The reference the
 * sanitizer run checks against brute force; false: arguments the call refuses */
inline bool fir_host(const gpsbb_fir_t *f, const int16_t *w, long nsamp, const int16_t *hist_in, int16_t *hist_out, int16_t *y, uint64_t *clipped)
{
    if (!fir_ok(f) || !w || !y || nsamp < 1 || nsamp % f->decim)
        return false;
    const int T = f->ntaps, D = f->decim;
    uint64_t clips = 0;
    for (long m = 0; m < nsamp / D; m++)
        for (int c = 0; c < 2; c++) {
            int32_t acc = 0;
            for (int k = 0; k < T; k++) {
                const long n = m * D + D - 1 - k; /* >= -(T - 1) */
                const int32_t x = n >= 0 ? w[2 * n + c] : (hist_in ? hist_in[2 * (T - 1 + n) + c] : 0);
                acc += (int32_t)f->h[k] * x;
            }
            const int32_t r = fir_round(acc, f->shift), v = fir_clamp(r);
            clips += v != r;
            y[2 * m + c] = (int16_t)v;
        }
    if (hist_out) {
        int16_t tail[2 * GPSBB_FIR_MAX_TAPS];
        for (int i = 0; i < T - 1; i++) {
            const long n = nsamp - (T - 1) + i;
            for (int c = 0; c < 2; c++)
                tail[2 * i + c] = n >= 0 ? w[2 * n + c] : (hist_in ? hist_in[2 * (T - 1 + n) + c] : 0);
        }
        memcpy(hist_out, tail, (size_t)(T - 1) * 4);
    }
    if (clipped)
        *clipped = clips;
    return true;
}

} /* namespace gpsbb_impl */
#endif
