/* Interference on the host-bound outputs (include/gpsbb.h, gpsbb_interf_t: the definition in full).  Up to four emitters — CW
 * tones and sawtooth chirps, each optionally pulsed — are added to the render where the noise is added, before the shift, the
 * saturation and the format's quantiser.  Every value is a pure function of the absolute sample position, in integer
 * arithmetic (gpsbb_interf.h: the statements the host's gpsbb_interf_eval runs too).  Noise and interference share one path out:
 * impair_unit_x / impair_sample_x make x = v + N + J of a 16-byte unit / of one sample for every kernel that needs it, and
 * k_impair_iq<FMT, NOISE, INTERF> is the one gather that applies either or both.  Hand-written HIP for gfx950. */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpsbb_interf.h"
#include "gpsbb_noise.hip.h"

namespace gpsbb_impl {

struct ImpairArgs {
    NoiseArgs nz;  /* sample0, shift and shift8 always; key and s256 with NOISE */
    InterfArgs it; /* it.sample0 == nz.sample0, it.shift == nz.shift */
};

/* the carrier tables in LDS: entry k = cos512[k] (low half) and sin512[k] (high half) as int16 */
struct InterfLdsTab {
    const uint32_t *t;
    __device__ __forceinline__ void operator()(uint32_t idx, int *c, int *s) const
    {
        const uint32_t v = t[idx];
        *c = (int)(v << 16) >> 16;
        *s = (int)v >> 16;
    }
};

__device__ __forceinline__ void interf_stage(uint32_t *cs, const int32_t *__restrict__ gtabs /* cos[512], sin[512] */, int tid, int nthr)
{
    for (int k = tid; k < 512; k += nthr)
        cs[k] = ((uint32_t)gtabs[k] & 0xffffu) | ((uint32_t)gtabs[512 + k] << 16);
}

/* J of the NS consecutive samples that start d samples after the launch's first: j[2 k] = J.I, j[2 k + 1] = J.Q of sample k.
 * One seek (the divisions by the sweep and the gate period, as multiplications) per emitter, then steps. */
template <int NS, class Tab>
__device__ __forceinline__ void interf_run(const InterfArgs &it, unsigned long long d, const Tab &tab, int *j)
{
#pragma unroll
    for (int k = 0; k < 2 * NS; k++)
        j[k] = 0;
#pragma unroll
    for (int e = 0; e < INTERF_MAX; e++) {
        if (e < it.n) { /* (uniform) */
            InterfPos p = interf_seek(it.e[e], it.sample0, d);
#pragma unroll
            for (int k = 0; k < NS; k++)
                interf_step(it.e[e], p, tab, j[2 * k], j[2 * k + 1]);
        }
    }
}

/* The 8 values x = v + N + J of step 4, before the shift, of the 4 samples at stream position s (an aligned 16-byte unit of the
 * source): the one place that makes them.  The gather shifts, saturates and stores them, k_level (gpsbb_level.hip.h) measures
 * them.  jj: the unit's J (zeros without a set).  ODD: s is odd, so the 4 samples straddle three Philox pairs */
template <bool ODD, bool NOISE>
__device__ __forceinline__ void impair_unit_x(gather_u32x4 q, unsigned long long s, const NoiseArgs &a, const int2 *tab, const int jj[8],
                                              int xo[8])
{
    uint32_t x[12];
    if (NOISE) {
        const unsigned long long m = s >> 1;
        noise_philox((uint32_t)m, (uint32_t)(m >> 32), a.key0, a.key1, x);
        noise_philox((uint32_t)(m + 1), (uint32_t)((m + 1) >> 32), a.key0, a.key1, x + 4);
        if (ODD)
            noise_philox((uint32_t)(m + 2), (uint32_t)((m + 2) >> 32), a.key0, a.key1, x + 8);
    }
    const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int c = (j & 1) ? (int)v[j >> 1] >> 16 : (int)(v[j >> 1] << 16) >> 16;
        xo[j] = c + jj[j] + (NOISE ? noise_n(x[(ODD ? 2 : 0) + j], tab, a.s256) : 0);
    }
}

/* The same of one sample, for whoever is not on a 16-byte unit (the gather's ragged tail and unaligned path, a block's head and
 * tail in k_level): N and J of the sample d samples after the launch's first, added to (xi, xq).  Tab: where the caller keeps the
 * carrier tables (InterfLdsTab).  k_despread's ds_view states the same sum once more: sharing this function cost two of its 36
 * instantiations two instructions each, and that kernel is hot. */
template <bool NOISE, bool INTERF, class Tab>
__device__ __forceinline__ void impair_sample_x(int &xi, int &xq, unsigned long long d, const ImpairArgs &a, const int2 *ntab, const Tab &tab)
{
    if (INTERF) {
        int j[2];
        interf_run<1>(a.it, d, tab, j);
        xi += j[0];
        xq += j[1];
    }
    if (NOISE) {
        const unsigned long long s = a.nz.sample0 + d;
        uint32_t x[4];
        noise_philox((uint32_t)(s >> 1), (uint32_t)(s >> 33), a.nz.key0, a.nz.key1, x);
        const bool odd = (s & 1ull) != 0ull; /* (selects: an indexed private array would go to scratch) */
        xi += noise_n(odd ? x[2] : x[0], ntab, a.nz.s256);
        xq += noise_n(odd ? x[3] : x[1], ntab, a.nz.s256);
    }
}

/* The gather with the impairments fused in: k_gather_to_host's / k_pack_iq's job on a wider grid.  The
 * slot (or fill, or device buffer) is one flat stream of n int16 components I0, Q0, I1, Q1 ... at positions sample0 + k / 2.  A
 * workgroup takes PACK_UNITS 16-byte loads per round, as k_pack_iq: SC16 stores 16 bytes per lane per load (a wavefront 1 KB
 * contiguous), SC8 8 bytes (512), SC1 one byte, transposed through LDS into 8 contiguous bytes per lane.  Per unit: with INTERF
 * one seek and four steps per emitter, with NOISE two or three Philox calls.  The knot table (NOISE) and the carrier tables
 * packed into 2 KB (INTERF) sit in LDS, each staged under its flag only.  src == dst (in place, SC16) is allowed: every lane
 * writes only what it has read.  A source not 16-byte aligned or a destination not aligned to its store takes a per-component
 * loop (same bytes), as does the ragged tail.  Step 4's saturations go to *nclip and SC8's own to *clip8, one atomic per workgroup
 * each.  Without either flag there is nothing to fuse: that is k_gather_to_host / k_pack_iq. */
template <int FMT, bool NOISE, bool INTERF>
__global__ __launch_bounds__(256) void k_impair_iq(const int16_t *src, void *dst, size_t n, ImpairArgs a, const int2 *__restrict__ gtab,
                                                   const int32_t *__restrict__ gcs, unsigned long long *__restrict__ nclip,
                                                   unsigned long long *__restrict__ clip8)
{
    static_assert(NOISE || INTERF, "the plain gather and pack are k_gather_to_host and k_pack_iq");
    __shared__ int2 tab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint32_t cs[INTERF ? 512 : 1];
    __shared__ __attribute__((aligned(16))) unsigned char t1[FMT == PACK_SC1 ? PACK_UNITS : 16];
    __shared__ uint32_t wsum[2][4];
    const int tid = (int)threadIdx.x;
    if (NOISE)
        for (int i = tid; i < NOISE_KNOTS - 1; i += 256)
            tab[i] = gtab[i];
    if (INTERF)
        interf_stage(cs, gcs, tid, 256);
    __syncthreads();
    uint32_t cl = 0, cl8 = 0;
    const size_t nunits = n / 8;
    const uintptr_t dalign = FMT == NOISE_SC16 ? 15 : 7;
    unsigned char *const db = reinterpret_cast<unsigned char *>(dst);
    /* component k of the source (sample k / 2, I or Q) through step 4 */
    auto comp = [&](size_t k) {
        int xi = src[k], xq = xi;
        impair_sample_x<NOISE, INTERF>(xi, xq, (unsigned long long)(k >> 1), a, tab, InterfLdsTab{cs});
        return noise_apply((k & 1) ? xq : xi, 0, a.nz.shift, cl);
    };
    if ((((uintptr_t)src & 15) | ((uintptr_t)dst & dalign)) == 0) {
        const gather_u32x4 *sv = reinterpret_cast<const gather_u32x4 *>(src);
        const size_t nchunk = (nunits + PACK_UNITS - 1) / PACK_UNITS;
        const bool odd = (a.nz.sample0 & 1) != 0;
        for (size_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
            const size_t u0 = c * PACK_UNITS + (size_t)tid;
            gather_u32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (u0 + (size_t)u * 256 < nunits)
                    v[u] = __builtin_nontemporal_load(sv + u0 + (size_t)u * 256);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const size_t q = u0 + (size_t)u * 256;
                if (q < nunits) {
                    int w[8], jj[8];
                    if (INTERF) {
                        interf_run<4>(a.it, 4ull * q, InterfLdsTab{cs}, jj);
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; j++)
                            jj[j] = 0;
                    }
                    const unsigned long long s = a.nz.sample0 + 4ull * q;
                    if (odd)
                        impair_unit_x<true, NOISE>(v[u], s, a.nz, tab, jj, w);
                    else
                        impair_unit_x<false, NOISE>(v[u], s, a.nz, tab, jj, w);
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        w[j] = noise_apply(w[j], 0, a.nz.shift, cl);
                    if (FMT == NOISE_SC16) {
                        gather_u32x4 o;
                        o.x = ((uint32_t)w[0] & 0xffffu) | (uint32_t)w[1] << 16;
                        o.y = ((uint32_t)w[2] & 0xffffu) | (uint32_t)w[3] << 16;
                        o.z = ((uint32_t)w[4] & 0xffffu) | (uint32_t)w[5] << 16;
                        o.w = ((uint32_t)w[6] & 0xffffu) | (uint32_t)w[7] << 16;
                        __builtin_nontemporal_store(o, reinterpret_cast<gather_u32x4 *>(dst) + q);
                    } else if (FMT == PACK_SC8) {
                        pack_u32x2 o;
                        o.x = noise_sc8(w[0], a.nz.shift8, cl8) | noise_sc8(w[1], a.nz.shift8, cl8) << 8 |
                              noise_sc8(w[2], a.nz.shift8, cl8) << 16 | noise_sc8(w[3], a.nz.shift8, cl8) << 24;
                        o.y = noise_sc8(w[4], a.nz.shift8, cl8) | noise_sc8(w[5], a.nz.shift8, cl8) << 8 |
                              noise_sc8(w[6], a.nz.shift8, cl8) << 16 | noise_sc8(w[7], a.nz.shift8, cl8) << 24;
                        __builtin_nontemporal_store(o, reinterpret_cast<pack_u32x2 *>(dst) + q);
                    } else {
                        uint32_t r = 0;
#pragma unroll
                        for (int j = 0; j < 8; j++)
                            r |= (uint32_t)(w[j] > 0) << (7 - j);
                        t1[u * 256 + tid] = (unsigned char)r;
                    }
                }
            }
            if (FMT == PACK_SC1) {
                __syncthreads();
                const size_t b0 = c * PACK_UNITS + 8 * (size_t)tid;
                if (b0 + 8 <= nunits) {
                    const pack_u32x2 o = *reinterpret_cast<const pack_u32x2 *>(t1 + 8 * tid);
                    __builtin_nontemporal_store(o, reinterpret_cast<pack_u32x2 *>(db + b0));
                } else {
                    for (size_t b = b0; b < nunits; b++)
                        db[b] = t1[b - c * PACK_UNITS];
                }
                __syncthreads();
            }
        }
        /* SC16 / SC8: the last n % 8 components of a ragged source (SC1 has none: nsamp % 4 == 0) */
        if (FMT != PACK_SC1 && blockIdx.x == 0 && (size_t)tid < n - nunits * 8) {
            const size_t k = nunits * 8 + (size_t)tid;
            const int w = comp(k);
            if (FMT == NOISE_SC16)
                reinterpret_cast<int16_t *>(dst)[k] = (int16_t)w;
            else
                db[k] = (unsigned char)noise_sc8(w, a.nz.shift8, cl8);
        }
    } else {
        const size_t nout = FMT == PACK_SC1 ? nunits : n;
        for (size_t k = (size_t)blockIdx.x * 256 + (size_t)tid; k < nout; k += (size_t)gridDim.x * 256) {
            if (FMT == NOISE_SC16) {
                reinterpret_cast<int16_t *>(dst)[k] = (int16_t)comp(k);
            } else if (FMT == PACK_SC8) {
                db[k] = (unsigned char)noise_sc8(comp(k), a.nz.shift8, cl8);
            } else {
                uint32_t r = 0;
                for (int j = 0; j < 8; j++)
                    r = r << 1 | (uint32_t)(comp(8 * k + (size_t)j) > 0);
                db[k] = (unsigned char)r;
            }
        }
    }
    /* the saturations: reduced per wavefront, one atomic per workgroup and counter */
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cl += (uint32_t)__shfl_down((int)cl, off);
        cl8 += (uint32_t)__shfl_down((int)cl8, off);
    }
    if ((tid & 63) == 0) {
        wsum[0][tid >> 6] = cl;
        wsum[1][tid >> 6] = cl8;
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long t = (unsigned long long)wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        if (t)
            atomicAdd(nclip, t);
        const unsigned long long t8 = (unsigned long long)wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
        if (FMT == PACK_SC8 && t8)
            atomicAdd(clip8, t8);
    }
}

} /* namespace gpsbb_impl */
