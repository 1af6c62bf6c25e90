/*
 * gpsbb_acq.h — the host-side rules of the acquisition search (include/gpsbb.h, gpsbb_device_acquire: the definition in full):
 * what a configuration may hold, the overflow bound, the steps from physical units, the best cell of a PRN's rows.  Plain C++,
 * no HIP: gpsbb.hip's entry points call these, tools/acq_asan.cpp runs them under the host sanitizers.
 */
#ifndef GPSBB_ACQ_H
#define GPSBB_ACQ_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gpsbb.h"

namespace gpsbb_impl {

constexpr int ACQ_PRNS = 32;
constexpr int ACQ_MAX_NCOH = 1 << 20, ACQ_MAX_LAGS = 32768, ACQ_MAX_NNC = 64, ACQ_MAX_SHIFT = 31;
constexpr uint64_t ACQ_MAX_CODE_STEP = 3ull << 31; /* 1.5 * 2^32 */

/* the format of a view as the despreader reads it: 0 SC16, 1 SC8 (*shift8), 2 SC1; -1: refused */
inline int acq_view_format(unsigned view, int *shift8)
{
    const unsigned f = (view & GPSBB_OUT_FORMAT_MASK) >> 8, sh = (view & GPSBB_OUT_SHIFT_MASK) >> 12;
    *shift8 = (int)sh;
    if ((view & ~(GPSBB_OUT_FORMAT_MASK | GPSBB_OUT_SHIFT_MASK)) || f > 2 || (sh && f != 1))
        return -1;
    return (int)f;
}

/* 2 * nnc * ((B >> a) + 1)^2 < 2^64 with B = N * Wmax * 1024 */
inline bool acq_fits(int fmt, int ncoh, int nnc, int a)
{
    const unsigned __int128 wmax = fmt == 0 ? 32768u : (fmt == 1 ? 128u : 1u);
    const unsigned __int128 B = (unsigned __int128)(uint64_t)ncoh * wmax * 1024u; /* <= 2^45 */
    const unsigned __int128 t = (B >> a) + 1;
    return (unsigned __int128)2 * (unsigned)nnc * t * t < ((unsigned __int128)1 << 64);
}

inline int acq_min_shift(unsigned view, int ncoh, int nnc)
{
    int sh8;
    const int fmt = acq_view_format(view, &sh8);
    if (fmt < 0 || ncoh < 1 || ncoh > ACQ_MAX_NCOH || nnc < 1 || nnc > ACQ_MAX_NNC)
        return GPSBB_E_BADARG;
    for (int a = 0; a <= ACQ_MAX_SHIFT; a++)
        if (acq_fits(fmt, ncoh, nnc, a))
            return a;
    return GPSBB_E_BADARG; /* (not reached: a = 31 fits every legal N and nnc) */
}

/* every field in range, the samples there, the bound kept; fmt: acq_view_format's */
inline bool acq_cfg_ok(const gpsbb_acq_cfg_t *c, int fmt, long nsamp)
{
    if (!c || fmt < 0 || c->prn_mask == 0u || c->nbins < 1 || c->nbins > GPSBB_ACQ_MAX_BINS || c->code_step == 0 ||
        c->code_step > ACQ_MAX_CODE_STEP || c->ncoh < 1 || c->ncoh > ACQ_MAX_NCOH || c->nlags < 1 || c->nlags > ACQ_MAX_LAGS || c->nnc < 1 ||
        c->nnc > ACQ_MAX_NNC || c->shift < 0 || c->shift > ACQ_MAX_SHIFT)
        return false;
    if ((long long)nsamp < (long long)c->nnc * c->ncoh + c->nlags - 1)
        return false;
    return acq_fits(fmt, c->ncoh, c->nnc, c->shift);
}

inline int acq_make(gpsbb_acq_cfg_t *cfg, double delt, double f_min_hz, double f_step_hz, int nbins, double coh_s, int nlags, int nnc,
                    unsigned view)
{
    int sh8;
    const int fmt = acq_view_format(view, &sh8);
    if (!cfg || fmt < 0 || !isfinite(delt) || !(delt > 0.0) || !isfinite(f_min_hz) || !isfinite(f_step_hz) || !isfinite(coh_s) ||
        !(coh_s > 0.0) || nbins < 1 || nbins > GPSBB_ACQ_MAX_BINS || nlags > ACQ_MAX_LAGS || nnc < 1 || nnc > ACQ_MAX_NNC)
        return GPSBB_E_BADARG;
    gpsbb_acq_cfg_t c;
    memset(&c, 0, sizeof c);
    c.prn_mask = 0xffffffffu;
    c.nbins = nbins;
    for (int k = 0; k < nbins; k++) {
        const double t = (f_min_hz + (double)k * f_step_hz) * delt;
        if (!(fabs(t) < 0.5))
            return GPSBB_E_BADARG;
        const double s = nearbyint(ldexp(t, 32)); /* |s| <= 2^31 */
        c.step[k] = (int32_t)(uint32_t)(int64_t)s;
    }
    const double cs = nearbyint(ldexp(1.023e6 * delt, 32));
    if (!(cs >= 1.0) || !(cs <= (double)ACQ_MAX_CODE_STEP))
        return GPSBB_E_BADARG;
    c.code_step = (uint64_t)cs;
    const double n = nearbyint(coh_s / delt);
    if (!(n >= 1.0) || !(n <= (double)ACQ_MAX_NCOH))
        return GPSBB_E_BADARG;
    c.ncoh = (int32_t)n;
    if (nlags <= 0) {
        const unsigned __int128 num = (unsigned __int128)1023 << 32;
        const unsigned __int128 per = (num + c.code_step - 1) / c.code_step;
        if (per > (unsigned)ACQ_MAX_LAGS)
            return GPSBB_E_BADARG;
        nlags = (int)per;
    }
    c.nlags = nlags;
    c.nnc = nnc;
    c.shift = acq_min_shift(view, c.ncoh, nnc);
    if (c.shift < 0)
        return GPSBB_E_BADARG;
    *cfg = c;
    return GPSBB_OK;
}

inline int acq_best(const gpsbb_acq_row_t *rows, const gpsbb_acq_cfg_t *cfg, int prn, int *bin, int *lag, uint64_t *peak, double *ratio)
{
    if (!rows || !cfg || prn < 1 || prn > ACQ_PRNS || cfg->nbins < 1 || cfg->nbins > GPSBB_ACQ_MAX_BINS || cfg->nlags < 1 ||
        cfg->nlags > ACQ_MAX_LAGS)
        return GPSBB_E_BADARG;
    const gpsbb_acq_row_t *r = rows + (size_t)(prn - 1) * (size_t)cfg->nbins;
    int best = 0;
    unsigned __int128 sum = 0;
    for (int k = 0; k < cfg->nbins; k++) {
        if (r[k].peak > r[best].peak)
            best = k;
        sum += ((unsigned __int128)r[k].sum_hi << 64) | r[k].sum_lo;
    }
    if (bin) *bin = best;
    if (lag) *lag = r[best].lag;
    if (peak) *peak = r[best].peak;
    if (ratio) {
        const double mean = (double)sum / ((double)cfg->nbins * (double)cfg->nlags);
        *ratio = mean > 0.0 ? (double)r[best].peak / mean : 0.0;
    }
    return GPSBB_OK;
}

} /* namespace gpsbb_impl */
#endif
