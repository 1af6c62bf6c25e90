/*
 * gpsbb_track.hip.h — k_track: the tracking loops of gpsbb_device_track (include/gpsbb.h has the definition in full; the rules that
 * need no GPU, the closing of an epoch among them, are gpsbb_track.h).  Hand-written HIP for gfx950.
 *
 *   one workgroup of four wavefronts per channel, and nothing between workgroups: no atomic, no flag, no spin.  A channel's
 *       feedback (this epoch's discriminators set the next epoch's steps) stays behind LDS and __syncthreads(), and the loop
 *       ends after at most max_epochs rounds.
 *   staged once: the carrier table as (cos, sin) int16 pairs (ds_view's table and the mixer's), the PRN's 1023 chips as 32 words,
 *       the noise's knots.
 *   an epoch: the lanes stride over its N samples, j = tid, tid + 256, ...: consecutive lanes read consecutive samples.  Per
 *       sample the view (ds_view, the despreader's), the mix, the three chips, six signed additions.  A term is below 2^25
 *       (Wmax * 1024), so 32 of them fit an int32; after at most 32 rounds the partials go into the lane's int64 sums: exact.
 *   the reduction: a butterfly over the wavefront's 64 lanes per sum, lane 0 of each wavefront to LDS, __syncthreads(), and
 *       thread 0 adds the four, closes the epoch (trk_close: steps 4-8, with the one int64 division per discriminator), writes
 *       the record and plans the next epoch (trk_plan: steps 1-2) into LDS; __syncthreads() again and every lane reads it.
 *   integer sums are order-free: the result does not depend on which lane took which sample.
 */
#ifndef GPSBB_TRACK_HIP_H
#define GPSBB_TRACK_HIP_H

#include "gpsbb_track.h"
#include "gpsbb_despread.hip.h"

namespace gpsbb_impl {

constexpr int TK_WG = 256;
constexpr int TK_WAVES = TK_WG / 64;
constexpr int TK_FLUSH = 32; /* rounds an int32 partial takes: 32 * 2^25 = 2^30 */

struct TrkArgs {
    DsArgs d;                   /* iq, shift8, nz, ntab, it: what ds_view reads */
    const int32_t *tabs;        /* cos512[512], sin512[512] */
    const uint32_t *ca_bits;    /* bit c & 31 of word prn * 32 + (c >> 5): chip c of the PRN */
    gpsbb_trk_cfg_t cfg;
    gpsbb_trk_state_t *states;  /* [nch], in and out */
    gpsbb_trk_epoch_t *epochs;  /* [nch][max_epochs] */
    int32_t *counts;            /* [nch] */
    long nsamp;
};

struct TrkLds {
    gpsbb_trk_state_t s;
    unsigned long long cs; /* the next epoch's code step and samples; go: it fits the buffer and the call's records */
    long long N;
    int count, go;
};

__device__ __forceinline__ void trk_next(const TrkArgs &a, TrkLds &L)
{
    uint64_t cs;
    int64_t N;
    trk_plan(a.cfg, L.s, &cs, &N);
    L.cs = cs;
    L.N = N;
    L.go = L.count < a.cfg.max_epochs && L.s.n0 + N <= (int64_t)a.nsamp;
}

__device__ __forceinline__ int trk_chip(const uint32_t *chips, unsigned long long phi)
{
    const uint32_t c = (uint32_t)(phi >> 32); /* < 1023 */
    return (int)((chips[c >> 5] >> (c & 31u)) & 1u);
}

template <int VIEW, bool NOISE, bool INTERF>
__global__ __launch_bounds__(TK_WG) void k_track(TrkArgs a)
{
    __shared__ uint2 rep[512]; /* .x = (cos, sin) as an int16 pair */
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint32_t chips[32];
    __shared__ long long red[TK_WAVES][6];
    __shared__ TrkLds L;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, ch = (int)blockIdx.x;
    for (int k = tid; k < 512; k += TK_WG)
        rep[k] = make_uint2(ds_pair(a.tabs[k], a.tabs[512 + k]), 0u);
    if (NOISE)
        for (int k = tid; k < NOISE_KNOTS - 1; k += TK_WG)
            ntab[k] = a.d.ntab[k];
    if (tid == 0) {
        L.s = a.states[ch];
        L.count = 0;
        trk_next(a, L);
    }
    __syncthreads();
    if (tid < 32)
        chips[tid] = a.ca_bits[L.s.prn * 32 + tid];
    __syncthreads();
    const unsigned long long spacing = a.cfg.spacing;
    for (int round = 0; round < a.cfg.max_epochs; round++) { /* (go is false after max_epochs records: the bound is said twice) */
        if (!L.go)
            break;
        const unsigned long long cs = L.cs, code_phase = L.s.code_phase;
        const long long n0 = L.s.n0;
        const int N = (int)L.N;
        const uint32_t s32 = (uint32_t)(int32_t)(L.s.carr_step >> 16), carr_phase = L.s.carr_phase;
        long long acc[6] = {0, 0, 0, 0, 0, 0};
        for (int j0 = tid; j0 < N; j0 += TK_WG * TK_FLUSH) {
            int part[6] = {0, 0, 0, 0, 0, 0};
            const int jend = min(N, j0 + TK_WG * TK_FLUSH);
            unsigned long long phi = code_phase + cs * (unsigned long long)j0; /* < LEN for j < N */
            uint32_t ph = carr_phase + s32 * (uint32_t)j0;
            for (int j = j0; j < jend; j += TK_WG, phi += cs * TK_WG, ph += s32 * TK_WG) {
                const long long n = n0 + j; /* < n0 + N <= nsamp */
                const uint32_t w = ds_view<VIEW, NOISE, INTERF>(a.d.iq[n], (unsigned long long)n, a.d, ntab, rep);
                const int wi = (int)(w << 16) >> 16, wq = (int)w >> 16;
                const uint32_t t = rep[ph >> 23].x;
                const int c = (int)(t << 16) >> 16, s = (int)t >> 16;
                const int yi = wi * c + wq * s, yq = wq * c - wi * s;
                unsigned long long pe = phi + spacing, pl = phi - spacing;
                pe -= pe >= TRK_LEN ? TRK_LEN : 0ull;
                pl += phi < spacing ? TRK_LEN : 0ull;
                const int xe = trk_chip(chips, pe), xp = trk_chip(chips, phi), xl = trk_chip(chips, pl);
                part[0] += xe ? yi : -yi;
                part[1] += xe ? yq : -yq;
                part[2] += xp ? yi : -yi;
                part[3] += xp ? yq : -yq;
                part[4] += xl ? yi : -yi;
                part[5] += xl ? yq : -yq;
            }
#pragma unroll
            for (int k = 0; k < 6; k++)
                acc[k] += part[k];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                acc[k] += __shfl_xor(acc[k], off);
            if (lane == 0)
                red[wave][k] = acc[k];
        }
        __syncthreads(); /* the four partials are there; every lane has read this epoch's plan */
        if (tid == 0) {
            int64_t sum[6];
            for (int k = 0; k < 6; k++) {
                long long v = 0;
                for (int w = 0; w < TK_WAVES; w++)
                    v += red[w][k];
                sum[k] = v;
            }
            gpsbb_trk_state_t st = L.s;
            gpsbb_trk_epoch_t rec;
            trk_close(a.cfg, st, cs, N, sum, &rec);
            a.epochs[(size_t)ch * (size_t)a.cfg.max_epochs + (size_t)L.count] = rec; /* count < max_epochs: go */
            L.s = st;
            L.count = L.count + 1;
            trk_next(a, L);
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.states[ch] = L.s;
        a.counts[ch] = L.count;
    }
}

} /* namespace gpsbb_impl */
#endif
