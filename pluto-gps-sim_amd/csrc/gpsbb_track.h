/*
 * gpsbb_track.h — the rules of the tracking loops (include/gpsbb.h, gpsbb_device_track: the definition in full) that do not need a
 * GPU: what a configuration and a state may hold, an epoch's geometry (steps 1-2), what closes an epoch (steps 4-8), the loop
 * constants from physical units, the seed from an acquisition hit, bit edge and bits from the records.  Plain C++: k_track's one
 * closing lane runs trk_plan and trk_close as they stand here, gpsbb.hip's entry points call the rest, tools/track_asan.cpp runs
 * all of it under the host sanitizers.
 */
#ifndef GPSBB_TRACK_H
#define GPSBB_TRACK_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gpsbb.h"

#if defined(__HIPCC__)
#define GPSBB_TRK_HD __host__ __device__ inline
#else
#define GPSBB_TRK_HD inline
#endif

namespace gpsbb_impl {

constexpr uint64_t TRK_LEN = 1023ull << 32;
constexpr uint64_t TRK_MAX_CODE_NOM = 3ull << 31; /* 1.5 * 2^32 */
constexpr int TRK_MAX_N = 1 << 20, TRK_MAX_EPOCHS = 1 << 20, TRK_MAX_CH = 32, TRK_MAX_EPOCH0 = 1 << 30;
constexpr int64_t TRK_CARR_MAX = (1ll << 47) - 1, TRK_CODE_INT_MAX = 1ll << 56, TRK_CODE_ADJ_MAX = 1ll << 49;

GPSBB_TRK_HD int64_t trk_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }
GPSBB_TRK_HD int64_t trk_sgn(int64_t x) { return x >= 0 ? 1 : -1; }
GPSBB_TRK_HD int64_t trk_abs(int64_t x) { return x >= 0 ? x : -x; }
/* m(x): the bit length of x for x >= 0, of ~x otherwise */
GPSBB_TRK_HD int trk_m(int64_t x)
{
    uint64_t y = (uint64_t)(x < 0 ? ~x : x);
    int n = 0;
    for (; y; y >>= 1)
        n++;
    return n;
}

/* steps 1 and 2: the code step of the next epoch and its samples */
GPSBB_TRK_HD void trk_plan(const gpsbb_trk_cfg_t &c, const gpsbb_trk_state_t &s, uint64_t *cs, int64_t *N)
{
    const int64_t nom = (int64_t)c.code_nom;
    const int64_t aid = c.aid_div ? s.carr_step / c.aid_div : 0;
    const int64_t v = trk_clamp(nom + aid + s.code_adj, nom - nom / 8, nom + nom / 8);
    *cs = (uint64_t)v;
    *N = (int64_t)((TRK_LEN - s.code_phase + (uint64_t)v - 1) / (uint64_t)v);
}

/* steps 4 to 8: the epoch's six sums (E.i, E.q, P.i, P.q, L.i, L.q) correlated at state s with cs and N close it: the record, and
 * s advanced */
GPSBB_TRK_HD void trk_close(const gpsbb_trk_cfg_t &c, gpsbb_trk_state_t &s, uint64_t cs, int64_t N, const int64_t sum[6], gpsbb_trk_epoch_t *rec)
{
    int mm = 0;
    for (int k = 0; k < 6; k++) {
        const int b = trk_m(sum[k]);
        mm = b > mm ? b : mm;
    }
    const int q = mm > 20 ? mm - 20 : 0;
    const int64_t Ei = sum[0] >> q, Eq = sum[1] >> q, Pi = sum[2] >> q, Pq = sum[3] >> q, Li = sum[4] >> q, Lq = sum[5] >> q;
    const int64_t E2 = Ei * Ei + Eq * Eq, L2 = Li * Li + Lq * Lq;
    const int64_t e_d = ((E2 - L2) * 16384) / (E2 + L2 + 1);
    const int mode = s.epoch < c.nfll ? 0 : 1;
    int64_t e_c = 0;
    const int64_t step_used = s.carr_step;
    if (mode == 0) {
        if (s.epoch > 0) {
            const int64_t cross = s.prev_i * Pq - s.prev_q * Pi, dot = s.prev_i * Pi + s.prev_q * Pq;
            e_c = (trk_sgn(dot) * cross * 16384) / (trk_abs(dot) + trk_abs(cross) + 1);
        }
        s.carr_int = trk_clamp(s.carr_int + (int64_t)c.kf * e_c, -TRK_CARR_MAX, TRK_CARR_MAX);
        s.carr_step = s.carr_int;
    } else {
        e_c = (trk_sgn(Pi) * Pq * 16384) / (trk_abs(Pi) + trk_abs(Pq) + 1);
        s.carr_int = trk_clamp(s.carr_int + (int64_t)c.kp2 * e_c, -TRK_CARR_MAX, TRK_CARR_MAX);
        s.carr_step = trk_clamp(s.carr_int + (int64_t)c.kp1 * e_c, -TRK_CARR_MAX, TRK_CARR_MAX);
    }
    s.code_int = trk_clamp(s.code_int + (int64_t)c.kd2 * e_d, -TRK_CODE_INT_MAX, TRK_CODE_INT_MAX);
    s.code_adj = (s.code_int + (int64_t)c.kd1 * e_d) >> 8;
    rec->n0 = s.n0;
    rec->N = (int32_t)N;
    rec->q = q;
    rec->e_i = sum[0];
    rec->e_q = sum[1];
    rec->p_i = sum[2];
    rec->p_q = sum[3];
    rec->l_i = sum[4];
    rec->l_q = sum[5];
    rec->carr_step = step_used;
    rec->code_phase = s.code_phase;
    rec->carr_phase = s.carr_phase;
    rec->e_c = (int32_t)e_c;
    rec->e_d = (int32_t)e_d;
    rec->mode = mode;
    const uint32_t s32 = (uint32_t)(int32_t)(step_used >> 16);
    s.carr_phase += s32 * (uint32_t)N;
    s.code_phase = s.code_phase + cs * (uint64_t)N - TRK_LEN;
    s.n0 += N;
    s.epoch += 1;
    s.prev_i = Pi;
    s.prev_q = Pq;
}

inline bool trk_cfg_ok(const gpsbb_trk_cfg_t *c)
{
    if (!c || c->code_nom == 0 || c->code_nom > TRK_MAX_CODE_NOM || c->spacing == 0 || c->nfll < 0 || c->max_epochs < 1 ||
        c->max_epochs > TRK_MAX_EPOCHS)
        return false;
    const uint64_t lo = c->code_nom - c->code_nom / 8;
    return lo > 0 && (TRK_LEN + lo - 1) / lo <= (uint64_t)TRK_MAX_N;
}

inline bool trk_state_ok(const gpsbb_trk_state_t *s, long nsamp)
{
    if (s->prn < 1 || s->prn > 32 || s->epoch < 0 || s->epoch > TRK_MAX_EPOCH0 || s->n0 < 0 || s->n0 > (int64_t)nsamp ||
        s->code_phase >= TRK_LEN || s->carr_int > TRK_CARR_MAX || s->carr_int < -TRK_CARR_MAX || s->carr_step > TRK_CARR_MAX ||
        s->carr_step < -TRK_CARR_MAX || s->code_int > TRK_CODE_INT_MAX || s->code_int < -TRK_CODE_INT_MAX ||
        s->code_adj > TRK_CODE_ADJ_MAX || s->code_adj < -TRK_CODE_ADJ_MAX)
        return false;
    return s->epoch == 0 || (trk_m(s->prev_i) <= 20 && trk_m(s->prev_q) <= 20);
}

inline bool trk_gain(double x, int32_t *k)
{
    const double r = nearbyint(x);
    if (!isfinite(r) || !(fabs(r) <= 2147483647.0))
        return false;
    *k = (int32_t)r;
    return true;
}

inline int trk_make(gpsbb_trk_cfg_t *cfg, double delt, double fll_gain, double pll_bw_hz, double dll_gain, int nfll, int max_epochs)
{
    if (!cfg || !isfinite(delt) || !(delt > 0.0) || !isfinite(fll_gain) || !isfinite(pll_bw_hz) || !isfinite(dll_gain) ||
        max_epochs > TRK_MAX_EPOCHS)
        return GPSBB_E_BADARG;
    if (!(fll_gain > 0.0)) fll_gain = 0.15;
    if (!(pll_bw_hz > 0.0)) pll_bw_hz = 15.0;
    if (!(dll_gain > 0.0)) dll_gain = 0.1;
    gpsbb_trk_cfg_t c;
    memset(&c, 0, sizeof c);
    const double cn = nearbyint(ldexp(1.023e6 * delt, 32));
    if (!(cn >= 1.0) || !(cn <= (double)TRK_MAX_CODE_NOM))
        return GPSBB_E_BADARG;
    c.code_nom = (uint64_t)cn;
    c.aid_div = 1540ll << 16;
    c.spacing = 1u << 31;
    c.nfll = nfll > 0 ? nfll : 100;
    c.max_epochs = max_epochs > 0 ? max_epochs : 1000;
    const double two_pi = 6.283185307179586, nper = (double)TRK_LEN / cn, T = nper * delt, wn = pll_bw_hz / 0.53;
    if (!trk_gain(fll_gain * 0x1p+34 / (two_pi * nper), &c.kf) || !trk_gain(wn * wn * T * delt / two_pi * 0x1p+34, &c.kp2) ||
        !trk_gain(1.414 * wn * T / (two_pi * nper) * 0x1p+34, &c.kp1) || !trk_gain(dll_gain * 0x1p+24 / nper, &c.kd1) || !trk_cfg_ok(&c))
        return GPSBB_E_BADARG;
    *cfg = c;
    return GPSBB_OK;
}

inline int trk_seed(gpsbb_trk_state_t *state, const gpsbb_acq_cfg_t *acq, int prn, int bin, int lag)
{
    if (!state || !acq || prn < 1 || prn > 32 || acq->nbins < 1 || acq->nbins > GPSBB_ACQ_MAX_BINS || bin < 0 || bin >= acq->nbins || lag < 0)
        return GPSBB_E_BADARG;
    memset(state, 0, sizeof *state);
    state->prn = prn;
    state->n0 = lag;
    state->carr_int = state->carr_step = (int64_t)acq->step[bin] * 65536;
    /* step -2^31 would give -2^47, one beyond the loop's range */
    state->carr_int = state->carr_step = trk_clamp(state->carr_step, -TRK_CARR_MAX, TRK_CARR_MAX);
    return GPSBB_OK;
}

inline int trk_bitsync(const gpsbb_trk_epoch_t *e, int n, int skip, int *offset, int32_t hist[20])
{
    if (!e || n < 0 || skip < 0)
        return GPSBB_E_BADARG;
    int32_t h[20] = {0};
    for (int k = skip + 1; k < n; k++)
        if ((e[k].p_i >= 0) != (e[k - 1].p_i >= 0))
            h[k % 20]++;
    int best = 0;
    for (int k = 1; k < 20; k++)
        if (h[k] > h[best])
            best = k;
    if (offset) *offset = best;
    if (hist) memcpy(hist, h, sizeof h);
    return GPSBB_OK;
}

inline int trk_bits(const gpsbb_trk_epoch_t *e, int n, int first, int8_t *bits, int max)
{
    if (!e || !bits || n < 0 || first < 0 || max < 0)
        return GPSBB_E_BADARG;
    int nb = 0;
    for (long k = first; k + 20 <= (long)n && nb < max; k += 20, nb++) {
        int64_t sum = 0; /* 20 sums below 2^45 */
        for (int j = 0; j < 20; j++)
            sum += e[k + j].p_i;
        bits[nb] = (int8_t)(sum >= 0 ? 1 : -1);
    }
    return nb;
}

} /* namespace gpsbb_impl */
#endif
