/*
 * gpsbb_despread_lags.hip.h — k_despread_lags: k_despread's correlation at a set of sample lags, not just lag 0
 * (include/gpsbb.h: gpsbb_batch_despread_lags has the definition).  What multipath does to a receiver is a correlation
 * function with a second peak; the prompt sum alone cannot show it.  Hand-written HIP for gfx950, beside k_despread, which
 * it shares the model, the danger test, the exact fallback and the replica image with (gpsbb_despread.hip.h).
 *
 *   lane = sample mod 64, tiles in chunks from a per-block counter: k_despread's map.
 *   the view is computed ONCE per sample, for the tile and a halo of 64 samples on either side: 18 groups of 64 instead of
 *       16 (a side is skipped when no lag looks that way).  Interference and noise of sample m are those of m's own stream
 *       position b * nsamp + m; a position outside [0, nsamp) is zero: a block does not see its neighbours.  The 1152 words
 *       go to the wavefront's own strip of LDS (4.5 KB, 18 KB per workgroup) and w[n + L] is read from there: consecutive
 *       lanes read consecutive words, whatever L is, so the reads are conflict-free.  Nothing is held in registers across
 *       the channel loop but the strip's address.
 *   the replica of a channel-sample is computed ONCE (k_despread's 37 instructions) and its 16 table entries of the tile
 *       stay in registers across the lags.  A sample whose model is in danger takes the exact replica IN PLACE before any
 *       sum is formed, so every lag's sum is exact; a sample n that does not exist (n >= nsamp) has a zero replica —
 *       its partner w[n + L] may well exist for L < 0.
 *   per lag a channel-sample then costs one LDS read and two v_dot2c_i32_i16: the 16 reads of a lag are issued together, the
 *       32 dot products follow.  The int32-per-lane bound holds per lag (a term is below 2^25.1, sixteen fit).
 *   sums: a butterfly per lag would cost more than the lag itself (six steps of four ds_bpermute on 64-bit values), so the
 *       16 values of a channel (lag l, component c: v = 2 l + c) are summed over the wavefront ONCE, through LDS: every lane
 *       parks its int32 partial of value v in row v of the wavefront's own 16 x 64 block (rows padded to 68 words), lane
 *       (v, q) = (lane & 15, lane >> 4) reads quarter q of row v as four 128-bit words and widens and adds its 16 numbers,
 *       and two butterfly steps over q finish it.  Lane (v, q) then keeps value v of the channels with (i & 3) == q, in
 *       register set i >> 2, while consecutive tiles share a segment, then one 64-bit integer atomic per (channel, segment,
 *       chunk, lag) and component.  Integer sums: the result does not depend on who took which chunk.
 *   the strip is private to its wavefront: LDS operations of one wavefront complete in order, so a wave barrier with a
 *       workgroup-scope fence (compiler ordering + s_waitcnt lgkmcnt(0)) is all that stands between writing the strip and
 *       reading it, and between the last read of a tile and the next tile's writes.
 */
#ifndef GPSBB_DESPREAD_LAGS_HIP_H
#define GPSBB_DESPREAD_LAGS_HIP_H

#include "gpsbb_despread.hip.h"

namespace gpsbb_impl {

constexpr int DSL_MAX_LAGS = GPSBB_DESPREAD_MAX_LAGS;
constexpr int DSL_HALO = GPSBB_DESPREAD_MAX_LAG;  /* one group of 64 on either side */
constexpr int DSL_STRIP = TILE + 2 * DSL_HALO;    /* words per wavefront */
constexpr int DSL_RED_ROW = 64 + 4;               /* words per row of the reduction block: rows 4 banks apart */
static_assert(DSL_HALO == 64 && 2 * DSL_MAX_LAGS == 16 && GPSBB_MAX_CHAN == 16,
              "one halo group per side; lane (v, q) = (2 * lag + component, channel & 3), register set channel >> 2");

struct DslArgs {
    DsArgs d;                /* out: [nblocks][nch][nseg][nlags][2] */
    int lags[DSL_MAX_LAGS];  /* each within +-DSL_HALO */
    int nlags;
    int halo_lo, halo_hi;    /* some lag is negative / positive: that side's halo is needed */
};

template <int VIEW, bool NOISE, int SG, bool INTERF = false>
__global__ __launch_bounds__(DS_WG) void k_despread_lags(BatchDev p, DslArgs al)
{
    __shared__ DsLds L;
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint32_t strip[DS_WAVES][DSL_STRIP];
    __shared__ __attribute__((aligned(16))) int red[DS_WAVES][2 * DSL_MAX_LAGS][DSL_RED_ROW];
    __shared__ int lagv[DSL_MAX_LAGS];
    const DsArgs &a = al.d;
    const int tid = (int)threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.wgs_per_block);
    if (b >= p.nblocks)
        return;
    const gpsbb_chan_t *__restrict__ cb = p.ch + (size_t)b * p.nch;
    const EvConst *__restrict__ kb = p.evc + (size_t)b * p.nch;
    /* ---- stage: k_despread's image, and the lags ---- */
    ds_stage<NOISE>(p, a, cb, tid, L, ntab);
    if (tid < DSL_MAX_LAGS)
        lagv[tid] = tid < al.nlags ? al.lags[tid] : 0;
    __syncthreads();

    /* ---- from here on every wavefront works alone ---- */
    const int lane = tid & 63;
    uint32_t *__restrict__ vw = strip[tid >> 6];
    int(*__restrict__ rd)[DSL_RED_ROW] = red[tid >> 6];
    const int rv = lane & 15, rq = lane >> 4; /* the value and the quarter of its row this lane sums; the channels it keeps */
    const uint32_t act_mask = ds_active(cb, p.nch, lane);
    const int nlags = al.nlags;
    const int ntw = p.ntiles, nst = SG ? p.nstates : ntw;
    const double *__restrict__ txb = p.tile_x + ev_tile_x_row((size_t)b, p.nch, 0, NCO_CODE, nst);
    const uint32_t *__restrict__ tnb = p.tile_nav + ev_tile_nav_row((size_t)b, p.nch, 0, nst);
    const uint32_t *__restrict__ iqb = a.iq + (size_t)b * p.nsamp;
    const double guard = 0x1p+20 + (double)PD_BAND * 0x1p-32;
    /* lane (v, q), set r: value v (lag v >> 1, component v & 1) of channel 4 r + q over the tiles of segment run_seg this
     * wavefront has taken */
    long long run[4] = {0, 0, 0, 0};
    int run_seg = -1;
    unsigned long long n_exact = 0ull;
    auto flush = [&]() {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = 4 * r + rq;
            if (run_seg >= 0 && i < p.nch && rv < 2 * nlags && run[r])
                atomicAdd(a.out + (((size_t)b * p.nch + i) * (size_t)a.nseg + (size_t)run_seg) * (size_t)(2 * nlags) + (size_t)rv,
                          (unsigned long long)run[r]);
            run[r] = 0;
        }
    };
    for (;;) {
        const int base = ds_claim(a, b, lane);
        if (base >= ntw)
            break;
        const int stop = base + a.chunk < ntw ? base + a.chunk : ntw;
        for (int wt = base; wt < stop; wt++) {
            const int seg = wt / a.seg_tiles;
            if (seg != run_seg) {
                flush();
                run_seg = seg;
            }
            /* ---- the strip: word k is the view of sample wt*TILE - 64 + k, zero where the block has no such sample ---- */
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); /* the last tile's reads have returned */
            __builtin_amdgcn_wave_barrier();
            const int m0 = wt * TILE - DSL_HALO + lane;
#pragma unroll 2
            for (int g = 0; g < SPT + 2; g++) {
                const int m = m0 + g * 64;
                const bool need = (g != 0 || al.halo_lo) && (g != SPT + 1 || al.halo_hi);
                uint32_t w = 0u;
                if (need && m >= 0 && m < p.nsamp)
                    w = ds_view<VIEW, NOISE, INTERF>(iqb[m], (unsigned long long)b * (unsigned long long)p.nsamp + (unsigned long long)m, a,
                                                     ntab, L.rep[0]);
                vw[g * 64 + lane] = w;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); /* the strip is written before any lane reads it */
            __builtin_amdgcn_wave_barrier();
            const int left = p.nsamp - wt * TILE - lane; /* samples j*64 < left exist */
            const EvStateAt cx = ev_state_at(SG, NCO_CODE, wt), cy = ev_state_at(SG, NCO_CARR, wt); /* SG is the code's granule */
            const int g = cx.entry, gy = cy.entry, ns = cx.since * TILE + lane, nsy = cy.since * TILE + lane;
            const double n0 = (double)ns, n0y = (double)nsy; /* samples since the state's */
            for (uint32_t mk = act_mask; mk; mk &= mk - 1) {
                const int i = __builtin_ctz(mk);
                const double S = scalar_load(&kb[i].S), sc = scalar_load(&kb[i].sc);
                const uint32_t down = scalar_load(&kb[i].down) != 0 ? 1u : 0u;
                const double xt_s = txb[ev_tile_x_row(0, p.nch, i, NCO_CODE, nst) + g], yt = txb[ev_tile_x_row(0, p.nch, i, NCO_CARR, nst) + gy];
                /* (a granule table's code states carry the data bits in their signs: ev_nav_in_sign) */
                const double xt = ev_nav_in_sign(SG) ? __builtin_fabs(xt_s) : xt_s;
                const uint32_t nav = ev_nav_in_sign(SG) ? ev_nav_of_signs(p, (size_t)b, i, g) : tnb[ev_tile_nav_row(0, p.nch, i, nst) + g];
                const double yg = (down ? 512.0 - yt : yt) + guard, xg = xt + guard;
                const uint32_t flip = down ? 511u : 0u;
                const uint32_t *chips = L.chips[i];
                /* ---- the replica of the lane's 16 samples, once ---- */
                uint2 t[SPT];
                uint32_t bad = 0u;
#pragma unroll
                for (int j = 0; j < SPT; j++) {
                    bool bj;
                    const uint32_t r = ds_model_sample(n0 + (double)(j * 64), n0y + (double)(j * 64), S, sc, yg, xg, flip, nav, chips, a.danger, bj);
                    const bool is = j * 64 < left;
                    bad |= bj && is ? 1u << j : 0u;
                    const uint2 tj = (&L.rep[0][0])[r];
                    t[j] = is ? tj : make_uint2(0u, 0u); /* a sample that does not exist correlates with nothing */
                }
                /* ---- rare: the samples whose model came within its error of an integer take the exact replica instead ---- */
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad != 0u) != 0ull, 0)) {
#pragma unroll 1
                    for (int j = 0; j < SPT; j++) { /* (one call site, the entry put back by selects: t[] stays in registers) */
                        if (!((bad >> j) & 1u))
                            continue;
                        const uint32_t re = ds_exact<SG>(xt, yt, S, sc, down, nav, ns + j * 64, nsy + j * 64, chips);
                        const uint2 te = (&L.rep[0][0])[re];
#pragma unroll
                        for (int q = 0; q < SPT; q++)
                            t[q] = q == j ? te : t[q];
                        n_exact++;
                    }
                }
                /* ---- per lag: 16 reads of the strip, then two dot products per sample; the lane's partials to its column ---- */
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); /* the last channel's block has been read */
                __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                for (int l = 0; l < nlags; l++) {
                    const int lag = __builtin_amdgcn_readfirstlane(lagv[l]);
                    const uint32_t *__restrict__ wl = vw + (DSL_HALO + lane + lag);
                    uint32_t w[SPT];
#pragma unroll
                    for (int j = 0; j < SPT; j++)
                        w[j] = wl[j * 64];
                    __builtin_amdgcn_sched_barrier(0); /* (all in flight before the first is waited for) */
                    int pi = 0, pq = 0;
#pragma unroll
                    for (int j = 0; j < SPT; j++) {
                        pi = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, w[j]), __builtin_bit_cast(ds_s16x2, t[j].x), pi, false);
                        pq = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, w[j]), __builtin_bit_cast(ds_s16x2, t[j].y), pq, false);
                    }
                    rd[2 * l][lane] = pi;
                    rd[2 * l + 1][lane] = pq;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); /* the block is written before any lane reads it */
                __builtin_amdgcn_wave_barrier();
                /* ---- widen and sum over the wavefront: lane (v, q) takes quarter q of row v, two butterfly steps join the quarters ---- */
                long long tot = 0;
                if (rv < 2 * nlags) {
                    const int4 *__restrict__ row = reinterpret_cast<const int4 *>(&rd[rv][rq * 16]);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int4 x = row[k];
                        tot += (long long)x.x + (long long)x.y + (long long)x.z + (long long)x.w;
                    }
                }
                tot += __shfl_xor(tot, 16);
                tot += __shfl_xor(tot, 32);
                const long long mine = (i & 3) == rq ? tot : 0ll;
#pragma unroll
                for (int r = 0; r < 4; r++)
                    run[r] += (i >> 2) == r ? mine : 0ll;
            }
        }
    }
    flush();
    ds_count_exact(a, lane, n_exact);
}

} /* namespace gpsbb_impl */
#endif
