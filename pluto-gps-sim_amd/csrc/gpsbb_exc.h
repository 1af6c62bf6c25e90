/*
 * gpsbb_exc.h — the rules of the interference excision (include/gpsbb.h, gpsbb_device_excise: the definition in full) that do not
 * need a GPU: what a gpsbb_exc_t may hold, the decision, the reduce step, the conjugate twiddle product and the butterfly of one
 * inverse radix-2 step, the overlap-add with its clamp, the two host functions that make a plan, and the whole definition in plain C
 * over view samples in host memory.  The load, the forward product and butterfly and the table are the power spectrum's
 * (gpsbb_psd.h).  Plain C++: k_excise decides, reduces, multiplies, adds and clamps with exc_zeroed, exc_reduce, exc_tmul, exc_bfly
 * and exc_ola as they stand here, gpsbb.hip's entry points call the rest, tools/exc_asan.cpp runs all of it under the host sanitizers.
 */
#ifndef GPSBB_EXC_H
#define GPSBB_EXC_H

#include <algorithm>
#include <vector>

#include "gpsbb_psd.h"

namespace gpsbb_impl {

constexpr int EXC_MIN_LOG2N = PSD_MIN_LOG2N, EXC_MAX_LOG2N = PSD_MAX_LOG2N, EXC_WIN_ONE = 16384;
static_assert((1 << EXC_MAX_LOG2N) == GPSBB_EXC_MAX_N && GPSBB_EXC_MAX_N == GPSBB_PSD_MAX_N, "the spectrum's transform");

/* G of the definition: the bits the reduce step takes; S = 13 - G are the overlap-add's */
GPSBB_PSD_HD int exc_g(int log2n) { return (log2n + 1) >> 1; }

/* decide: a set mask bit, or a power above a threshold that is on */
GPSBB_PSD_HD bool exc_zeroed(psd_c X, bool masked, uint64_t thr)
{
    const int64_t a = X.re, b = X.im;
    return masked || (thr != 0 && (uint64_t)(a * a) + (uint64_t)(b * b) > thr);
}

/* sgn(x) ((|x| + 2^(g - 1)) >> g): halves away from zero on both sides, |x| < 2^31 - 2^(g - 1) */
GPSBB_PSD_HD int32_t exc_round(int32_t x, int g)
{
    const uint32_t m = x < 0 ? 0u - (uint32_t)x : (uint32_t)x, r = (m + (1u << (g - 1))) >> g;
    return x < 0 ? -(int32_t)r : (int32_t)r;
}

GPSBB_PSD_HD psd_c exc_reduce(psd_c X, int g) { return psd_c{exc_round(X.re, g), exc_round(X.im, g)}; }

/* t = v * (c + i s) of the inverse: the conjugate of psd_tmul's twiddle, rounded alike */
GPSBB_PSD_HD psd_c exc_tmul(psd_c v, int32_t c, int32_t s)
{
    const int64_t re = (int64_t)v.re * c - (int64_t)v.im * s + ((int64_t)1 << 29);
    const int64_t im = (int64_t)v.im * c + (int64_t)v.re * s + ((int64_t)1 << 29);
    return psd_c{(int32_t)(re >> 30), (int32_t)(im >> 30)};
}

/* u, v <- u + t, u - t: no halving; every modulus stays below 2^28.5 plus rounding (include/gpsbb.h, the bound) */
GPSBB_PSD_HD void exc_bfly(psd_c &u, psd_c &v, psd_c t)
{
    const psd_c p{u.re + t.re, u.im + t.im};
    v = psd_c{u.re - t.re, u.im - t.im};
    u = p;
}

/* one component of the overlap-add: clamp((a + b + 2^(S - 1)) >> S), clips counts what the clamp changed */
GPSBB_PSD_HD int32_t exc_ola(int32_t a, int32_t b, int S, uint32_t &clips)
{
    const int32_t o = (a + b + (1 << (S - 1))) >> S, q = o < -32768 ? -32768 : (o > 32767 ? 32767 : o);
    clips += q != o;
    return q;
}

/* a legal window: 0 <= win[n] <= 16384 and win[n] + win[n + H] == 16384 */
inline bool exc_win_ok(const int16_t *win, int N)
{
    for (int n = 0; n < N / 2; n++)
        if (win[n] < 0 || win[n] > EXC_WIN_ONE || (int)win[n] + (int)win[n + N / 2] != EXC_WIN_ONE)
            return false;
    return true;
}

/* a plan and a length the call serves */
inline bool exc_ok(const gpsbb_exc_t *e, long nsamp)
{
    if (!e || e->log2n < EXC_MIN_LOG2N || e->log2n > EXC_MAX_LOG2N)
        return false;
    const long H = 1L << (e->log2n - 1);
    return nsamp >= H && nsamp % H == 0 && exc_win_ok(e->win, 1 << e->log2n);
}

inline bool exc_masked(const gpsbb_exc_t *e, int k) { return (e->mask[k >> 3] >> (k & 7)) & 1; }

inline int exc_make(gpsbb_exc_t *e, int log2n)
{
    if (!e || log2n < EXC_MIN_LOG2N || log2n > EXC_MAX_LOG2N)
        return GPSBB_E_BADARG;
    gpsbb_exc_t o;
    memset(&o, 0, sizeof o);
    o.log2n = log2n;
    const int N = 1 << log2n, H = N / 2;
    const double w = 2.0 * 3.14159265358979323846 / (double)N;
    for (int n = 0; n < H; n++) {
        o.win[n] = (int16_t)nearbyint(16384.0 * 0.5 * (1.0 - cos(w * (double)n)));
        o.win[n + H] = (int16_t)(EXC_WIN_ONE - o.win[n]);
    }
    *e = o;
    return GPSBB_OK;
}

/* the mask and the threshold from a spectrum of gpsbb_device_psd (SC16, the same log2n); e is changed only where GPSBB_OK */
inline int exc_from_psd(gpsbb_exc_t *e, const uint64_t *psd, const gpsbb_psd_t *p, long nseg, double mask_db, double thr_db)
{
    if (!e || !psd || !p || e->log2n < EXC_MIN_LOG2N || e->log2n > EXC_MAX_LOG2N || p->log2n != e->log2n || p->shift < 0 ||
        p->shift > PSD_MAX_SHIFT || nseg < 1 || nseg > PSD_MAX_NSEG || !std::isfinite(mask_db) || !std::isfinite(thr_db))
        return GPSBB_E_BADARG;
    const int N = 1 << e->log2n;
    std::vector<uint64_t> v(psd, psd + N);
    std::nth_element(v.begin(), v.begin() + (N - 1) / 2, v.end());
    const double med = (double)v[(N - 1) / 2];
    uint64_t thr = 0;
    if (thr_db > 0.0) {
        const double t = floor(ldexp(pow(10.0, thr_db / 10.0) * med, 2 * p->shift) / (double)nseg);
        if (!std::isfinite(t) || !(t < 0x1p+64))
            return GPSBB_E_BADARG;
        thr = (uint64_t)t;
    }
    uint8_t mask[GPSBB_EXC_MAX_N / 8];
    memset(mask, 0, sizeof mask);
    if (mask_db > 0.0) {
        const double lim = pow(10.0, mask_db / 10.0) * med;
        if (!std::isfinite(lim))
            return GPSBB_E_BADARG;
        for (int k = 0; k < N; k++)
            if ((double)psd[k] > lim)
                mask[k >> 3] |= (uint8_t)(1u << (k & 7));
    }
    memcpy(e->mask, mask, sizeof mask);
    e->thr = thr;
    return GPSBB_OK;
}

/* The definition in plain C over view samples w [nsamp][2] in host memory (already impaired): out [nsamp][2], hist_out [N][2] (may
 * be hist_in).  hist_in: [N][2] or NULL (zeros).  work: [N] psd_c, half: [N / 2] psd_c.  peak, where given: the largest
 * |component| any inverse step produced (the bound's witness).  false: arguments the call refuses */
inline bool exc_host(const gpsbb_exc_t *e, const int16_t *w, long nsamp, const int16_t *hist_in, const int32_t *c, const int32_t *s, psd_c *work,
                     psd_c *half, int16_t *out, int16_t *hist_out, uint64_t *clipped, uint64_t *excised, int64_t *peak = nullptr)
{
    if (!exc_ok(e, nsamp) || !w || !c || !s || !work || !half || !out)
        return false;
    const int L = e->log2n, N = 1 << L, H = N / 2, G = exc_g(L), S = 13 - G;
    const long nblk = nsamp / H;
    uint64_t exc = 0;
    uint32_t clips = 0;
    uint64_t clip_total = 0;
    int64_t pk = 0;
    for (long sg = 0; sg <= nblk; sg++) {
        const long base = (sg - 2) * (long)H;
        for (int n = 0; n < N; n++) {
            const long i = base + n; /* < nsamp */
            int32_t wi = 0, wq = 0;
            if (i >= 0) {
                wi = w[2 * i];
                wq = w[2 * i + 1];
            } else if (hist_in) {
                wi = hist_in[2 * (i + N)];
                wq = hist_in[2 * (i + N) + 1];
            }
            uint32_t r = 0;
            for (int b = 0; b < L; b++)
                r |= (((uint32_t)n >> b) & 1u) << (L - 1 - b);
            work[r] = psd_c{psd_load(wi, e->win[n], 1), psd_load(wq, e->win[n], 1)};
        }
        for (int m = 2; m <= N; m <<= 1) {
            const int h = m / 2;
            for (int j0 = 0; j0 < N; j0 += m)
                for (int j = 0; j < h; j++) {
                    const int k = j * (4096 / m);
                    psd_bfly(work[j0 + j], work[j0 + j + h], psd_tmul(work[j0 + j + h], c[k], s[k]));
                }
        }
        /* decide and reduce in natural bin order, then a[bitrev(k)] = Z[k]: an in-place swap of the pairs */
        for (int k = 0; k < N; k++) {
            const bool z = exc_zeroed(work[k], exc_masked(e, k), e->thr);
            exc += z && sg >= 1;
            work[k] = z ? psd_c{0, 0} : exc_reduce(work[k], G);
        }
        for (int k = 0; k < N; k++) {
            uint32_t r = 0;
            for (int b = 0; b < L; b++)
                r |= (((uint32_t)k >> b) & 1u) << (L - 1 - b);
            if ((int)r > k)
                std::swap(work[k], work[r]);
        }
        for (int m = 2; m <= N; m <<= 1) {
            const int h = m / 2;
            for (int j0 = 0; j0 < N; j0 += m)
                for (int j = 0; j < h; j++) {
                    const int k = j * (4096 / m);
                    exc_bfly(work[j0 + j], work[j0 + j + h], exc_tmul(work[j0 + j + h], c[k], s[k]));
                    if (peak)
                        for (const psd_c &q : {work[j0 + j], work[j0 + j + h]})
                            pk = std::max(pk, std::max<int64_t>(q.re < 0 ? -(int64_t)q.re : q.re, q.im < 0 ? -(int64_t)q.im : q.im));
                }
        }
        if (sg >= 1)
            for (int n = 0; n < H; n++) {
                clips = 0;
                out[2 * ((sg - 1) * (long)H + n)] = (int16_t)exc_ola(half[n].re, work[n].re, S, clips);
                out[2 * ((sg - 1) * (long)H + n) + 1] = (int16_t)exc_ola(half[n].im, work[n].im, S, clips);
                clip_total += clips;
            }
        for (int n = 0; n < H; n++)
            half[n] = work[n + H];
    }
    if (hist_out) {
        if (nsamp >= N)
            memcpy(hist_out, w + 2 * (nsamp - N), (size_t)N * 4);
        else { /* nsamp == H */
            if (hist_in)
                memmove(hist_out, hist_in + 2 * H, (size_t)H * 4);
            else
                memset(hist_out, 0, (size_t)H * 4);
            memcpy(hist_out + 2 * H, w, (size_t)H * 4);
        }
    }
    if (clipped)
        *clipped = clip_total;
    if (excised)
        *excised = exc;
    if (peak)
        *peak = pk;
    return true;
}

} /* namespace gpsbb_impl */
#endif
