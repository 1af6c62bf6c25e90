/* Receiver noise on the host-bound outputs (include/gpsbb.h, gpsbb_noise_t: the definition in full).  Every noise value is a pure
 * function of the seed and the absolute sample position — Philox4x32-10 of the pair index, a Q16 normal deviate from a knot
 * table — so that any split of a stream over calls, rings and shards, and every output format, sees the same noise at the same
 * sample.  k_noise_iq<FMT> does the job of k_gather_to_host / k_pack_iq with the noise fused in, on a wider grid. */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpsbb_kernels.hip.h"

namespace gpsbb_impl {

constexpr int NOISE_KNOTS = 1665; /* GPSBB_NOISE_KNOTS */
constexpr int NOISE_SC16 = 0;     /* k_noise_iq's int16 format; PACK_SC8 / PACK_SC1 as k_pack_iq */

struct NoiseArgs {
    uint32_t key0, key1;        /* lo32 / hi32 of the seed */
    unsigned long long sample0; /* stream position of component 0 of the launch's source */
    int s256;                   /* round(256 * sigma) */
    int shift;                  /* the noise shift, 0..7 */
    int shift8;                 /* SC8's own shift */
};

/* Philox4x32-10 with counter (c0, c1, 0, 0) (Salmon et al., SC'11) */
__device__ __forceinline__ void noise_philox(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t *x)
{
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0;
    x[1] = c1;
    x[2] = c2;
    x[3] = c3;
}

/* u -> sigma * z rounded (steps 2 and 3).  tab[i] = (K[i], K[i + 1] - K[i]) */
__device__ __forceinline__ int noise_n(uint32_t u, const int2 *tab, int s256)
{
    const uint32_t t = 0x7fffffffu - (u & 0x7fffffffu);
    const int e = 31 - __clz((int)(t | 64u)); /* floor(log2 t), 6 below 128 */
    const int g = e - 6;
    const uint32_t r = t & ((1u << g) - 1u);
    const int f = (int)(g <= 16 ? r << (16 - g) : r >> (g - 16));
    const int i = t < 64u ? (int)t : 64 * (e - 5) + (int)((t >> g) & 63u);
    const int2 k = tab[i];
    const int a = k.x + ((k.y * f + 32768) >> 16);
    const int z = (int)u < 0 ? -a : a;
    return (int)(((long long)s256 * z + (1ll << 23)) >> 24);
}

/* step 4: w = sat16((v + N) >> shift) */
__device__ __forceinline__ int noise_apply(int v, int n, int shift, uint32_t &clip)
{
    const int s = (v + n) >> shift;
    const int w = min(max(s, -32768), 32767);
    clip += w != s;
    return w;
}

/* the 8 components of the 4 samples at stream position s (an aligned 16-byte unit of the source), with noise.  ODD: s is odd,
 * so the 4 samples straddle three Philox pairs */
template <bool ODD>
__device__ __forceinline__ void noise_unit(gather_u32x4 q, unsigned long long s, const NoiseArgs &a, const int2 *tab, int w[8],
                                           uint32_t &clip)
{
    uint32_t x[12];
    const unsigned long long m = s >> 1;
    noise_philox((uint32_t)m, (uint32_t)(m >> 32), a.key0, a.key1, x);
    noise_philox((uint32_t)(m + 1), (uint32_t)((m + 1) >> 32), a.key0, a.key1, x + 4);
    if (ODD)
        noise_philox((uint32_t)(m + 2), (uint32_t)((m + 2) >> 32), a.key0, a.key1, x + 8);
    const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int c = (j & 1) ? (int)v[j >> 1] >> 16 : (int)(v[j >> 1] << 16) >> 16;
        w[j] = noise_apply(c, noise_n(x[(ODD ? 2 : 0) + j], tab, a.s256), a.shift, clip);
    }
}

/* one component k of the source (sample k / 2, I or Q), with noise: the ragged tail and the unaligned path */
__device__ __forceinline__ int noise_comp(int v, size_t k, const NoiseArgs &a, const int2 *tab, uint32_t &clip)
{
    const unsigned long long s = a.sample0 + (unsigned long long)(k >> 1);
    uint32_t x[4];
    noise_philox((uint32_t)(s >> 1), (uint32_t)(s >> 33), a.key0, a.key1, x);
    return noise_apply(v, noise_n(x[2 * (int)(s & 1) + (int)(k & 1)], tab, a.s256), a.shift, clip);
}

__device__ __forceinline__ uint32_t noise_sc8(int w, int shift8, uint32_t &clip8)
{
    const int s = w >> shift8;
    const int c = min(max(s, -128), 127);
    clip8 += c != s;
    return (uint32_t)c & 0xffu;
}

/* The slot (or fill, or device buffer) is one flat stream of n int16 components I0, Q0, I1, Q1 ... at positions sample0 + k / 2.
 * A workgroup takes PACK_UNITS 16-byte loads per round, as k_pack_iq: SC16 stores 16 bytes per lane per load (a wavefront 1 KB
 * contiguous), SC8 8 bytes (512), SC1 one byte, transposed through LDS into 8 contiguous bytes per lane.  The knot table sits in
 * LDS.  src == dst (in place, SC16) is allowed: every lane writes only the unit it has read.  A source not 16-byte aligned or a
 * destination not aligned to its store takes a per-component loop (same bytes).  Noise saturations go to *nclip and SC8's own
 * to *clip8, one atomic per workgroup each. */
template <int FMT>
__global__ __launch_bounds__(256) void k_noise_iq(const int16_t *src, void *dst, size_t n, NoiseArgs a, const int2 *__restrict__ gtab,
                                                  unsigned long long *__restrict__ nclip, unsigned long long *__restrict__ clip8)
{
    __shared__ int2 tab[NOISE_KNOTS - 1];
    __shared__ __attribute__((aligned(16))) unsigned char t1[FMT == PACK_SC1 ? PACK_UNITS : 16];
    __shared__ uint32_t wsum[2][4];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < NOISE_KNOTS - 1; i += 256)
        tab[i] = gtab[i];
    __syncthreads();
    uint32_t cl = 0, cl8 = 0;
    const size_t nunits = n / 8;
    const uintptr_t dalign = FMT == NOISE_SC16 ? 15 : 7;
    unsigned char *const db = reinterpret_cast<unsigned char *>(dst);
    if ((((uintptr_t)src & 15) | ((uintptr_t)dst & dalign)) == 0) {
        const gather_u32x4 *sv = reinterpret_cast<const gather_u32x4 *>(src);
        const size_t nchunk = (nunits + PACK_UNITS - 1) / PACK_UNITS;
        const bool odd = (a.sample0 & 1) != 0;
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
                    int w[8];
                    const unsigned long long s = a.sample0 + 4ull * q;
                    if (odd)
                        noise_unit<true>(v[u], s, a, tab, w, cl);
                    else
                        noise_unit<false>(v[u], s, a, tab, w, cl);
                    if (FMT == NOISE_SC16) {
                        gather_u32x4 o;
                        o.x = ((uint32_t)w[0] & 0xffffu) | (uint32_t)w[1] << 16;
                        o.y = ((uint32_t)w[2] & 0xffffu) | (uint32_t)w[3] << 16;
                        o.z = ((uint32_t)w[4] & 0xffffu) | (uint32_t)w[5] << 16;
                        o.w = ((uint32_t)w[6] & 0xffffu) | (uint32_t)w[7] << 16;
                        __builtin_nontemporal_store(o, reinterpret_cast<gather_u32x4 *>(dst) + q);
                    } else if (FMT == PACK_SC8) {
                        pack_u32x2 o;
                        o.x = noise_sc8(w[0], a.shift8, cl8) | noise_sc8(w[1], a.shift8, cl8) << 8 |
                              noise_sc8(w[2], a.shift8, cl8) << 16 | noise_sc8(w[3], a.shift8, cl8) << 24;
                        o.y = noise_sc8(w[4], a.shift8, cl8) | noise_sc8(w[5], a.shift8, cl8) << 8 |
                              noise_sc8(w[6], a.shift8, cl8) << 16 | noise_sc8(w[7], a.shift8, cl8) << 24;
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
            const int w = noise_comp(src[k], k, a, tab, cl);
            if (FMT == NOISE_SC16)
                reinterpret_cast<int16_t *>(dst)[k] = (int16_t)w;
            else
                db[k] = (unsigned char)noise_sc8(w, a.shift8, cl8);
        }
    } else {
        const size_t nout = FMT == PACK_SC1 ? nunits : n;
        for (size_t k = (size_t)blockIdx.x * 256 + (size_t)tid; k < nout; k += (size_t)gridDim.x * 256) {
            if (FMT == NOISE_SC16) {
                reinterpret_cast<int16_t *>(dst)[k] = (int16_t)noise_comp(src[k], k, a, tab, cl);
            } else if (FMT == PACK_SC8) {
                db[k] = (unsigned char)noise_sc8(noise_comp(src[k], k, a, tab, cl), a.shift8, cl8);
            } else {
                uint32_t r = 0;
                for (int j = 0; j < 8; j++)
                    r |= (uint32_t)(noise_comp(src[8 * k + (size_t)j], 8 * k + (size_t)j, a, tab, cl) > 0) << (7 - j);
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
