/* Interference on the host-bound outputs (include/gpsbb.h, gpsbb_interf_t: the definition in full).  Up to four emitters — CW
 * tones and sawtooth chirps, each optionally pulsed — are added to the render where the noise is added, before the shift, the
 * saturation and the format's quantiser.  Every value is a pure function of the absolute sample position, in integer
 * arithmetic (gpsbb_interf.h: the statements the host's gpsbb_interf_eval runs too).  k_impair_iq<FMT, NOISE> is k_noise_iq<FMT>
 * with J added and the noise optional; k_noise_iq itself, and every launch of it, is untouched.  Hand-written HIP for gfx950. */
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

/* noise_unit with J: the 8 components of the 4 samples at stream position s, w = sat16((v + N + J) >> shift) */
template <bool ODD, bool NOISE>
__device__ __forceinline__ void impair_unit(gather_u32x4 q, unsigned long long s, const NoiseArgs &a, const int2 *tab, const int jj[8],
                                            int w[8], uint32_t &clip)
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
        w[j] = noise_apply(c + jj[j], NOISE ? noise_n(x[(ODD ? 2 : 0) + j], tab, a.s256) : 0, a.shift, clip);
    }
}

/* impair_unit stopped before the shift: the 8 values x = v + N + J of step 4 (k_level measures them, gpsbb_level.hip.h) */
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

/* noise_comp with J: one component k of the source (the ragged tail and the unaligned path) */
template <bool NOISE>
__device__ __forceinline__ int impair_comp(int v, size_t k, const ImpairArgs &a, const int2 *tab, const uint32_t *cs, uint32_t &clip)
{
    int j[2];
    interf_run<1>(a.it, (unsigned long long)(k >> 1), InterfLdsTab{cs}, j);
    int n = 0;
    if (NOISE) {
        const unsigned long long s = a.nz.sample0 + (unsigned long long)(k >> 1);
        uint32_t x[4];
        noise_philox((uint32_t)(s >> 1), (uint32_t)(s >> 33), a.nz.key0, a.nz.key1, x);
        const uint32_t u = (s & 1) ? ((k & 1) ? x[3] : x[2]) : ((k & 1) ? x[1] : x[0]); /* (selects: no indexed private array) */
        n = noise_n(u, tab, a.nz.s256);
    }
    return noise_apply(v + ((k & 1) ? j[1] : j[0]), n, a.nz.shift, clip);
}

/* k_noise_iq's shape, line for line (gpsbb_noise.hip.h has the account): 16-byte units, PACK_UNITS of them per workgroup and
 * round, SC16 / SC8 stored straight from the lane, SC1 transposed through LDS, the ragged tail and the unaligned path per
 * component, src == dst allowed for SC16.  Added: the carrier tables packed into 2 KB of LDS, and per unit and emitter one seek
 * and four steps.  The knot table is staged with NOISE only. */
template <int FMT, bool NOISE>
__global__ __launch_bounds__(256) void k_impair_iq(const int16_t *src, void *dst, size_t n, ImpairArgs a, const int2 *__restrict__ gtab,
                                                   const int32_t *__restrict__ gcs, unsigned long long *__restrict__ nclip,
                                                   unsigned long long *__restrict__ clip8)
{
    __shared__ int2 tab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint32_t cs[512];
    __shared__ __attribute__((aligned(16))) unsigned char t1[FMT == PACK_SC1 ? PACK_UNITS : 16];
    __shared__ uint32_t wsum[2][4];
    const int tid = (int)threadIdx.x;
    if (NOISE)
        for (int i = tid; i < NOISE_KNOTS - 1; i += 256)
            tab[i] = gtab[i];
    interf_stage(cs, gcs, tid, 256);
    __syncthreads();
    uint32_t cl = 0, cl8 = 0;
    const size_t nunits = n / 8;
    const uintptr_t dalign = FMT == NOISE_SC16 ? 15 : 7;
    unsigned char *const db = reinterpret_cast<unsigned char *>(dst);
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
                    interf_run<4>(a.it, 4ull * q, InterfLdsTab{cs}, jj);
                    const unsigned long long s = a.nz.sample0 + 4ull * q;
                    if (odd)
                        impair_unit<true, NOISE>(v[u], s, a.nz, tab, jj, w, cl);
                    else
                        impair_unit<false, NOISE>(v[u], s, a.nz, tab, jj, w, cl);
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
            const int w = impair_comp<NOISE>(src[k], k, a, tab, cs, cl);
            if (FMT == NOISE_SC16)
                reinterpret_cast<int16_t *>(dst)[k] = (int16_t)w;
            else
                db[k] = (unsigned char)noise_sc8(w, a.nz.shift8, cl8);
        }
    } else {
        const size_t nout = FMT == PACK_SC1 ? nunits : n;
        for (size_t k = (size_t)blockIdx.x * 256 + (size_t)tid; k < nout; k += (size_t)gridDim.x * 256) {
            if (FMT == NOISE_SC16) {
                reinterpret_cast<int16_t *>(dst)[k] = (int16_t)impair_comp<NOISE>(src[k], k, a, tab, cs, cl);
            } else if (FMT == PACK_SC8) {
                db[k] = (unsigned char)noise_sc8(impair_comp<NOISE>(src[k], k, a, tab, cs, cl), a.nz.shift8, cl8);
            } else {
                uint32_t r = 0;
                for (int j = 0; j < 8; j++)
                    r |= (uint32_t)(impair_comp<NOISE>(src[8 * k + (size_t)j], 8 * k + (size_t)j, a, tab, cs, cl) > 0) << (7 - j);
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
