/*
 * gpsbb_blank.hip.h — k_blank: the pulse blanker of gpsbb_device_blank (include/gpsbb.h has the definition in full; the rules that
 * need no GPU, the geometry among them, are gpsbb_blank.h).  Hand-written HIP for gfx950.  The counts of the workgroups are added
 * by k_exc_fold (gpsbb_exc.hip.h), which asks nothing of them but to be pairs.
 *
 *   a workgroup of four wavefronts takes a run of consecutive tiles of BLANK_TILE = 4096 outputs, one tile after the other, and
 *       nothing passes between workgroups: no atomics, two counts per workgroup for the fold.
 *   staged once per tile: the view (ds_view, the despreader's: a pure function of the position) of the tile's samples and of the
 *       K = G + hold + L - 1 before them — the delay G makes the window causal, nothing behind the tile is wanted — as one dword
 *       (Q << 16 | I) per sample, consecutive lanes consecutive samples.  Halo samples inside the buffer are recomputed (K / 4096
 *       of the views twice: 0.6 % at L = G = hold = 8, 33 % at the ranges' end), samples before the buffer come from the uploaded
 *       history.  Only the samples are kept, 4 bytes each: p is two multiplications away, and (4096 + 1341) * 4 = 21.2 KB leaves
 *       room for seven workgroups on a CU.
 *   boxcar: the tile's trigger bits, G + hold before its first output and one per output, are shared out R consecutive ones per
 *       lane (blank_share).  A lane adds the L powers of its first window and then slides, s += p[new] - p[old] in uint64, exact:
 *       L + 2 R LDS reads for R bits in place of L R.  R is odd, so the lanes' reads, R dwords apart, fall into 32 different
 *       banks per 32 lanes: no padding, no swizzle, conflict-free by the bank rule (a / 4) mod 32 (not from a counter run).
 *   dilation without a loop over hold: a lane's R bits are one mask word; the exclusive prefix count of the lanes' popcounts
 *       (a wavefront scan by shifts, the four wavefronts' totals through LDS) and the mask give C(q), the triggers before bit q,
 *       from two LDS reads, and output o is blanked iff C(o + G + hold + 1) - C(o) > 0.  Consecutive lanes read the same or the
 *       next entry: broadcasts.  The blanked count falls out of the same test, the trigger count out of the popcounts of the
 *       bits the tile owns (those of its outputs: the G + hold before are an earlier tile's, or the history's).
 *   stores: one dword per lane, consecutive lanes consecutive samples; plain.  Non-temporal stores (a.nt, which only the
 *       experiments build can set) took the same time to the microsecond when alternated with them.
 *   the compiler's report (profiles/bl01_resource_usage.txt): plain 50 VGPRs, with noise 67, with emitters 116 to 120; no scratch.
 *   the history tail (the last K samples of hist_in ++ w) is written by the lanes that stage those samples as their tile's own,
 *       and by tile 0 for what survives of hist_in when nsamp < K.
 *   integer sums are order-free: the result does not depend on the launch's shape.
 */
#ifndef GPSBB_BLANK_HIP_H
#define GPSBB_BLANK_HIP_H

#include "gpsbb_blank.h"
#include "gpsbb_despread.hip.h"

namespace gpsbb_impl {

inline size_t blank_lds_bytes(int K) { return (size_t)(BLANK_TILE + K) * sizeof(uint32_t); }

struct BlankArgs {
    DsArgs d;                 /* iq, nz, ntab, it: what ds_view reads */
    const int32_t *tabs;      /* cos512[512], sin512[512] (INTERF) */
    const uint32_t *hist_in;  /* [K] samples (Q << 16 | I) */
    uint32_t *hist_out;       /* [K] */
    uint32_t *out;            /* [nsamp] */
    unsigned long long *part; /* [nwg][2]: blanked, triggers */
    unsigned long long thr;
    long nsamp, run;
    int L, G, hold, K, R, nt; /* nt: store the output non-temporally (the experiments build's knob; 0 in the product) */
    uint32_t rcp;             /* ceil(2^BLANK_RCP_BITS / R) */
};

/* the triggers before bit q: q <= BLANK_WG * R, so that q / R <= BLANK_WG, where base holds the total and mask nothing */
__device__ __forceinline__ uint32_t blank_before(uint32_t q, const BlankArgs &a, const uint32_t *base, const uint32_t *mask)
{
    const uint32_t t = (q * a.rcp) >> BLANK_RCP_BITS, r = q - t * (uint32_t)a.R; /* q / R, q mod R; r < 32 */
    return base[t] + (uint32_t)__popc(mask[t] & ((1u << r) - 1u));
}

template <bool NOISE, bool INTERF>
__global__ __launch_bounds__(BLANK_WG) void k_blank(BlankArgs a)
{
    extern __shared__ uint32_t blank_w[]; /* BLANK_TILE + K samples */
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint2 rep[INTERF ? 512 : 1]; /* .x = (cos, sin) as an int16 pair: ds_view's table */
    __shared__ uint32_t base[BLANK_WG + 1], mask[BLANK_WG + 1], wtot[BLANK_WG / 64];
    __shared__ unsigned long long red[2][BLANK_WG / 64];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (INTERF)
        for (int k = tid; k < 512; k += BLANK_WG)
            rep[k] = make_uint2(ds_pair(a.tabs[k], a.tabs[512 + k]), 0u);
    if (NOISE)
        for (int k = tid; k < NOISE_KNOTS - 1; k += BLANK_WG)
            ntab[k] = a.d.ntab[k];
    const int L = a.L, K = a.K, R = a.R, D = a.G + a.hold;
    const long tail0 = a.nsamp - K; /* the history handed on begins here */
    const long t0 = (long)blockIdx.x * a.run;
    uint32_t nblank = 0u, ntrig = 0u; /* a lane's counts: at most run * 16 and run * R */

    if (blockIdx.x == 0 && tail0 < 0) /* nsamp < K: the end of hist_in is the beginning of the history handed on */
        for (long i = tid; i < -tail0; i += BLANK_WG)
            a.hist_out[i] = a.hist_in[i + a.nsamp];

    for (long tile = t0; tile < t0 + a.run; tile++) {
        const long m0 = tile * BLANK_TILE;
        if (m0 >= a.nsamp)
            break;
        const int outs = (int)min((long)BLANK_TILE, a.nsamp - m0); /* 1 .. BLANK_TILE */
        const int W = outs + K, J = outs + D;                      /* samples staged, trigger bits */
        __syncthreads(); /* the tables are there; the tile before has been read */

        /* ---- stage: window sample i is w[m0 - K + i] ---- */
        for (int i = tid; i < W; i += BLANK_WG) {
            const long n = m0 - K + i; /* in [-K, nsamp) */
            uint32_t x;
            if (n >= 0)
                x = ds_view<DS_SC16, NOISE, INTERF>(a.d.iq[n], (unsigned long long)n, a.d, ntab, rep);
            else
                x = a.hist_in[K + n];
            blank_w[i] = x;
            if (i >= K && n >= tail0)
                a.hist_out[n - tail0] = x; /* n < nsamp: an index below K */
        }
        __syncthreads();

        /* ---- boxcar: bit q is trig[m0 - D + q], its window the samples q .. q + L - 1 ---- */
        const int q0 = tid * R, q1 = min(q0 + R, J);
        uint32_t bits = 0u;
        if (q0 < J) {
            unsigned long long s = 0ull;
            for (int k = 0; k < L; k++)
                s += blank_pow(blank_w[q0 + k]); /* q0 + L - 1 < J + L - 1 = W */
            bits = s > a.thr;
            for (int q = q0 + 1; q < q1; q++) {
                s += blank_pow(blank_w[q + L - 1]); /* <= J - 1 + L - 1 < W */
                s -= blank_pow(blank_w[q - 1]);
                bits |= (uint32_t)(s > a.thr) << (q - q0);
            }
            /* the bits of the tile's own samples: q >= D */
            const int own = D - q0;
            ntrig += (uint32_t)__popc(own <= 0 ? bits : (own >= R ? 0u : bits & ~((1u << own) - 1u)));
        }
        /* ---- the exclusive prefix count of the lanes' popcounts ---- */
        const uint32_t cnt = (uint32_t)__popc(bits);
        uint32_t inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)inc, o);
            if (lane >= o)
                inc += v;
        }
        if (lane == 63)
            wtot[wave] = inc;
        __syncthreads();
        uint32_t before = 0u;
        for (int k = 0; k < wave; k++)
            before += wtot[k];
        base[tid] = before + inc - cnt;
        mask[tid] = bits;
        if (tid == BLANK_WG - 1) {
            base[BLANK_WG] = before + inc;
            mask[BLANK_WG] = 0u;
        }
        __syncthreads();

        /* ---- outputs: o is blanked iff a trigger lies in bits o .. o + D; else it is w[m0 + o - G], window sample o + hold + L - 1 ---- */
        for (int o = tid; o < outs; o += BLANK_WG) {
            const bool z = blank_before((uint32_t)(o + D + 1), a, base, mask) != blank_before((uint32_t)o, a, base, mask); /* o + D + 1 <= J <= 256 R */
            nblank += z;
            const uint32_t v = z ? 0u : blank_w[o + a.hold + L - 1]; /* below outs + K = W; m0 + o < nsamp */
            if (a.nt)
                __builtin_nontemporal_store(v, a.out + m0 + o);
            else
                a.out[m0 + o] = v;
        }
    }

    /* ---- the counts ---- */
    unsigned long long c0 = nblank, c1 = ntrig;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        c0 += (unsigned long long)__shfl_xor((int)(uint32_t)c0, o) & 0xffffffffull;
        c1 += (unsigned long long)__shfl_xor((int)(uint32_t)c1, o) & 0xffffffffull;
    }
    if (lane == 0) {
        red[0][wave] = c0;
        red[1][wave] = c1;
    }
    __syncthreads();
    if (tid < 2) {
        unsigned long long s = 0ull;
        for (int k = 0; k < BLANK_WG / 64; k++)
            s += red[tid][k];
        a.part[2 * (size_t)blockIdx.x + (size_t)tid] = s;
    }
}

} /* namespace gpsbb_impl */
#endif
