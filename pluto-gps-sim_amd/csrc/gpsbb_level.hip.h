/* The level of the host-bound output before its two shifts (include/gpsbb.h, gpsbb_level_t: the definition in full).  For every
 * block, the histogram of the bit length m(x) of x = v + N + J — step 4's value before the shift — and the exact sum of x^2, per
 * component.  The histogram decides both clip counters for every (shift, shift8) (gpsbb_level_clips), so one pass over the render
 * chooses them (gpsbb_level_choose).  k_level<NOISE, INTERF> has k_impair_iq's read side — the same impair_unit_x and
 * impair_sample_x make its x — and stores no samples: noise and emitters are regenerated at their absolute positions.
 * Hand-written HIP for gfx950. */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpsbb_interf.hip.h"

namespace gpsbb_impl {

constexpr int LEVEL_CLASSES = 32; /* GPSBB_LEVEL_CLASSES */
constexpr int LEVEL_COPIES = 16;  /* LDS words per wavefront, component and class: lane l counts in copy l & 15 */

struct LevelOut { /* gpsbb_level_t */
    unsigned long long n, sumsq[2], hist[2][LEVEL_CLASSES];
};

/* m(x): the bit length of x for x >= 0, of ~x otherwise (0 for 0 and -1; 24 at most here) */
__device__ __forceinline__ int level_class(int x)
{
    return 32 - __clz(x ^ (x >> 31));
}

/* one component into the wavefront's histogram and the lane's sum of squares.  A wavefront's components fall into three to six
 * classes: with one word per class 64 lanes would queue on it, with LEVEL_COPIES words four lanes do, and the copies of a class
 * lie in 16 different banks. */
__device__ __forceinline__ void level_add(uint32_t *hw /* [LEVEL_CLASSES][LEVEL_COPIES] of this component */, int x, int lane,
                                          unsigned long long &sq)
{
    atomicAdd(&hw[level_class(x) * LEVEL_COPIES + (lane & (LEVEL_COPIES - 1))], 1u);
    sq += (unsigned long long)((long long)x * (long long)x);
}

/* nblocks blocks of nsamp int16 pairs at src (4-byte aligned), block b at stream position a.nz.sample0 + b * nsamp.  The grid is a
 * flattened (block, chunk) list, cpb chunks of PACK_UNITS 16-byte units per block, walked by at most one workgroup per CU.  Blocks
 * are 4 * nsamp bytes apart, so each has a head and a tail of up to three samples off the 16-byte grid of the buffer: chunk 0
 * takes them one sample per lane.  The units in between are k_impair_iq's: non-temporal 16-byte loads, eight in flight per lane,
 * one seek and four steps per emitter, two or three Philox calls by the parity of the unit's ABSOLUTE position (which changes
 * from block to block when nsamp is odd).  Per item the wavefronts' histograms and sums meet in LDS and leave with 64-bit vector
 * atomics into out[b] (zeroed by the caller): integers, so the result does not depend on the order.  Nothing else is stored. */
template <bool NOISE, bool INTERF>
__global__ __launch_bounds__(256) void k_level(const int16_t *src, long nblocks, int nsamp, int cpb, ImpairArgs a,
                                               const int2 *__restrict__ gtab, const int32_t *__restrict__ gcs, LevelOut *out)
{
    __shared__ int2 tab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint32_t cs[INTERF ? 512 : 1];
    __shared__ uint32_t hist[4 * 2 * LEVEL_CLASSES * LEVEL_COPIES]; /* [wavefront][component][class][copy]: 16 KB */
    __shared__ unsigned long long wsq[4][2];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (NOISE)
        for (int i = tid; i < NOISE_KNOTS - 1; i += 256)
            tab[i] = gtab[i];
    if (INTERF)
        interf_stage(cs, gcs, tid, 256);
    for (int i = tid; i < 4 * 2 * LEVEL_CLASSES * LEVEL_COPIES; i += 256)
        hist[i] = 0u;
    __syncthreads();
    uint32_t *const hi = hist + (wv * 2 + 0) * LEVEL_CLASSES * LEVEL_COPIES;
    uint32_t *const hq = hist + (wv * 2 + 1) * LEVEL_CLASSES * LEVEL_COPIES;
    const long long off = (long long)(((uintptr_t)src >> 2) & 3); /* sample g of the buffer starts a unit when (g + off) % 4 == 0 */
    const long long nitems = (long long)nblocks * cpb;
    for (long long w = blockIdx.x; w < nitems; w += gridDim.x) {
        const long long b = w / cpb;
        const int c = (int)(w - b * cpb);
        const long long g0 = b * nsamp, g1 = g0 + nsamp;
        long long gh = ((g0 + off + 3) & ~3ll) - off; /* the block's first sample on the grid ... */
        gh = gh < g1 ? gh : g1;
        long long gt = ((g1 + off) & ~3ll) - off;     /* ... and the end of its last whole unit */
        gt = gt > gh ? gt : gh;
        const long long nu = (gt - gh) >> 2;
        unsigned long long sqi = 0, sqq = 0;
        const gather_u32x4 *sv = reinterpret_cast<const gather_u32x4 *>(src + 2 * gh);
        const long long u0 = (long long)c * PACK_UNITS + tid;
        const bool odd = ((a.nz.sample0 + (unsigned long long)gh) & 1) != 0;
        gather_u32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (u0 + u * 256 < nu)
                v[u] = __builtin_nontemporal_load(sv + u0 + u * 256);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const long long q = u0 + u * 256;
            if (q < nu) {
                int x[8], jj[8];
                const unsigned long long d = (unsigned long long)(gh + 4 * q);
                if (INTERF) {
                    interf_run<4>(a.it, d, InterfLdsTab{cs}, jj);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        jj[k] = 0;
                }
                if (odd)
                    impair_unit_x<true, NOISE>(v[u], a.nz.sample0 + d, a.nz, tab, jj, x);
                else
                    impair_unit_x<false, NOISE>(v[u], a.nz.sample0 + d, a.nz, tab, jj, x);
#pragma unroll
                for (int k = 0; k < 8; k += 2) {
                    level_add(hi, x[k], lane, sqi);
                    level_add(hq, x[k + 1], lane, sqq);
                }
            }
        }
        if (c == 0) {
            /* head [g0, gh) and tail [gt, g1): six samples at most, one per lane of the first wavefront */
            const long long nh = gh - g0, nt = g1 - gt;
            if (tid < nh + nt) {
                const long long g = tid < nh ? g0 + tid : gt + (tid - nh);
                const uint32_t v = reinterpret_cast<const uint32_t *>(src)[g];
                int xi = (int)(v << 16) >> 16, xq = (int)v >> 16;
                impair_sample_x<NOISE, INTERF>(xi, xq, (unsigned long long)g, a, tab, InterfLdsTab{cs});
                level_add(hi, xi, lane, sqi);
                level_add(hq, xq, lane, sqq);
            }
        }
        /* the sums of squares over the wavefront, then everything over the workgroup */
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sqi += __shfl_down(sqi, o);
            sqq += __shfl_down(sqq, o);
        }
        if (lane == 0) {
            wsq[wv][0] = sqi;
            wsq[wv][1] = sqq;
        }
        __syncthreads();
        {
            /* thread t owns the 16 copies of (wavefront t / 64, component (t / 32) & 1, class t & 31): words [16 t, 16 t + 16) */
            uint32_t *p = hist + tid * LEVEL_COPIES;
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < LEVEL_COPIES; i++) {
                const int r = (i + tid) & (LEVEL_COPIES - 1); /* (rotated: the lanes of a wavefront in different banks) */
                s += p[r];
                p[r] = 0u;
            }
            if (s)
                atomicAdd(&out[b].hist[(tid >> 5) & 1][tid & 31], (unsigned long long)s);
            if (tid < 2)
                atomicAdd(&out[b].sumsq[tid], wsq[0][tid] + wsq[1][tid] + wsq[2][tid] + wsq[3][tid]);
            if (tid == 2 && c == 0)
                atomicAdd(&out[b].n, (unsigned long long)nsamp);
        }
        __syncthreads();
    }
}

} /* namespace gpsbb_impl */
