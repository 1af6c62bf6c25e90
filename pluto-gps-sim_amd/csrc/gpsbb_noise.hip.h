/* Receiver noise on the host-bound outputs (include/gpsbb.h, gpsbb_noise_t: the definition in full).  Every noise value is a pure
 * function of the seed and the absolute sample position — Philox4x32-10 of the pair index, a Q16 normal deviate from a knot
 * table — so that any split of a stream over calls, rings and shards, and every output format, sees the same noise at the same
 * sample.  Here: the generator (Philox, the deviate) and the two quantisers.  The kernel that applies them on the way out, with
 * or without interference, is k_impair_iq (gpsbb_interf.hip.h). */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpsbb_kernels.hip.h"

namespace gpsbb_impl {

constexpr int NOISE_KNOTS = 1665; /* GPSBB_NOISE_KNOTS */
constexpr int NOISE_SC16 = 0;     /* k_impair_iq's int16 format; PACK_SC8 / PACK_SC1 as k_pack_iq */

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

__device__ __forceinline__ uint32_t noise_sc8(int w, int shift8, uint32_t &clip8)
{
    const int s = w >> shift8;
    const int c = min(max(s, -128), 127);
    clip8 += c != s;
    return (uint32_t)c & 0xffu;
}

} /* namespace gpsbb_impl */
