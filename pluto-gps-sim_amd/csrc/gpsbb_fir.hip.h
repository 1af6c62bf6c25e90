/*
 * gpsbb_fir.hip.h — k_fir: the front-end filter of gpsbb_device_fir (include/gpsbb.h has the definition in full; the rules that
 * need no GPU, the rounding among them, are gpsbb_fir.h).  Hand-written HIP for gfx950.
 *
 *   one workgroup of four wavefronts takes a tile of FIR_TILE = 256 consecutive outputs, one per lane, and nothing passes between
 *       workgroups but one 64-bit vector atomic per wavefront that clipped.
 *   staged once: the view (ds_view, the despreader's: a pure function of the position) of the tile's (outs - 1) * D + Te input
 *       samples, Te = T rounded up to even.  Halo samples inside the buffer are recomputed, samples before the buffer come from
 *       the uploaded history, and what lies before the history (the one sample an odd T is padded with) is zero: its tap is.
 *   the LDS image holds PAIRS, one per input sample r of the window: { (I[r], I[r+1]), (Q[r], Q[r+1]) } as two int16 pairs in
 *       a uint2 — every pair of neighbours at every offset, so that two taps of one component are one v_dot2c_i32_i16 whatever
 *       the parity of the sample a lane starts from (odd D, even T: no alignment case exists).  A lane gets its right-hand
 *       neighbour's sample by a wavefront shift, so each wavefront stages 63 pairs from 64 views: 1.6 % of the views twice.
 *   and it holds them POLYPHASE: pair r lies at slot (r mod D) * PL + r / D.  Lane mo's tap pair j reads r = mo * D + c_j,
 *       c_j = Te - 2 - 2 j, that is slot mo + off_j with off_j = (c_j mod D) * PL + c_j / D the same for every lane: consecutive
 *       lanes read consecutive uint2, one conflict-free ds_read_b64 per two taps of both components, for every D.  A flat image
 *       would put the lanes 2 D dwords apart: 2-, 4-, 8- and 16-way conflicts for D = 2, 4, 8, 16.  PL is odd, which spreads
 *       the staging's writes (consecutive lanes, consecutive phases) over the banks.
 *   taps are uniform across lanes: packed pairs (h[2j+1], h[2j]) and the offsets off_j come in the kernel's arguments and are
 *       scalar operands.  Per output and component T / 2 dot products, T / 4 LDS reads.
 *   the history tail (the last T - 1 samples of hist_in ++ w) is written by the lanes that stage those samples as their tile's own
 *       (each input sample is owned by one tile), and by tile 0 for what survives of hist_in when nsamp < T - 1.
 *   integer sums are order-free: the result does not depend on the launch's shape.
 *   the compiler's report (profiles/fr01_resource_usage.txt): plain 23 VGPRs and no scratch, with noise 32 and none; the variants
 *       with emitters spill scalar registers (36 and 52 bytes of scratch per lane).  The conflict counts are from the bank rule
 *       (DESIGN.md 2.15 has the table of the three layouts), not from a counter run.
 */
#ifndef GPSBB_FIR_HIP_H
#define GPSBB_FIR_HIP_H

#include "gpsbb_fir.h"
#include "gpsbb_despread.hip.h"

namespace gpsbb_impl {

constexpr int FIR_WG = 256;
constexpr int FIR_TILE = FIR_WG;                          /* outputs of a tile: one per lane */
constexpr int FIR_MAX_PAIRS = (GPSBB_FIR_MAX_TAPS + 1) / 2; /* 65 */
constexpr int FIR_STAGE = (FIR_WG / 64) * 63;             /* pairs the workgroup stages per round */
constexpr int FIR_RCP_BITS = 20;                          /* r / D = (r * ceil(2^20 / D)) >> 20 for r < 2^13, D <= 16 */

/* the plane length of the polyphase image: the slots a phase needs, FIR_TILE + ceil((Te - 1) / D) at most, made odd */
inline int fir_plane(int Te, int D) { return (FIR_TILE + (Te + D - 2) / D + 1) | 1; }
/* bytes of the image */
inline size_t fir_lds_bytes(int Te, int D) { return (size_t)D * (size_t)fir_plane(Te, D) * sizeof(uint2); }

struct FirArgs {
    DsArgs d;                 /* iq, nz, ntab, it: what ds_view reads */
    const int32_t *tabs;      /* cos512[512], sin512[512] (INTERF) */
    const uint32_t *hist_in;  /* [T - 1] samples (Q << 16 | I) */
    uint32_t *hist_out;       /* [T - 1] */
    uint32_t *out;            /* [nsamp / D] */
    unsigned long long *clipped;
    long nsamp, nout;
    int T, Te, D, shift, PL, npairs;
    uint32_t rcp;             /* ceil(2^FIR_RCP_BITS / D) */
    uint32_t hp[FIR_MAX_PAIRS];  /* pair j: h[2j+1] (low half, times the earlier sample) and h[2j] (high half) */
    uint32_t off[FIR_MAX_PAIRS]; /* off_j */
};

template <bool NOISE, bool INTERF>
__global__ __launch_bounds__(FIR_WG) void k_fir(FirArgs a)
{
    extern __shared__ uint2 fir_img[]; /* D * PL pairs */
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint2 rep[INTERF ? 512 : 1]; /* .x = (cos, sin) as an int16 pair: ds_view's table */
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (INTERF)
        for (int k = tid; k < 512; k += FIR_WG)
            rep[k] = make_uint2(ds_pair(a.tabs[k], a.tabs[512 + k]), 0u);
    if (NOISE)
        for (int k = tid; k < NOISE_KNOTS - 1; k += FIR_WG)
            ntab[k] = a.d.ntab[k];
    if (NOISE || INTERF)
        __syncthreads();
    const long m0 = (long)blockIdx.x * FIR_TILE;              /* < nout */
    const int outs = (int)min((long)FIR_TILE, a.nout - m0);   /* 1 .. FIR_TILE */
    const int D = a.D, T = a.T;
    const long own_lo = m0 * D;                               /* the inputs from here to (m0 + outs) * D <= nsamp are this tile's own */
    const long ws = own_lo + D - a.Te;                        /* the window's first sample; its last is (m0 + outs) * D - 1 */
    const int NX = (outs - 1) * D + a.Te;                     /* samples of the window; pairs: NX - 1 */
    const long tail0 = a.nsamp - (T - 1);                     /* the history handed on begins here */

    /* ---- stage: wavefront w's lane l takes sample base + w * 63 + l; lane 63 only feeds lane 62 ---- */
    for (int base = 0; base < NX; base += FIR_STAGE) {
        const int r = base + wave * 63 + lane;
        const long n = ws + r;
        uint32_t x = 0u;
        if (r < NX) {
            if (n >= 0)
                x = ds_view<DS_SC16, NOISE, INTERF>(a.d.iq[n], (unsigned long long)n, a.d, ntab, rep); /* n < (m0 + outs) * D <= nsamp */
            else if (n >= -(long)(T - 1))
                x = a.hist_in[T - 1 + n];
        }
        const uint32_t nx = (uint32_t)__shfl_down((int)x, 1);
        if (lane < 63 && r < NX) {
            if (r < NX - 1) {
                const uint32_t q = ((uint32_t)r * a.rcp) >> FIR_RCP_BITS, p = (uint32_t)r - q * (uint32_t)D; /* r / D, r mod D */
                fir_img[p * (uint32_t)a.PL + q] = make_uint2((x & 0xffffu) | (nx << 16), (x >> 16) | (nx & 0xffff0000u));
            }
            if (n >= own_lo && n >= tail0)
                a.hist_out[n - tail0] = x; /* n < nsamp: an index below T - 1 */
        }
    }
    if (blockIdx.x == 0 && tail0 < 0) /* nsamp < T - 1: the end of hist_in is the beginning of the history handed on */
        for (long i = tid; i < -tail0; i += FIR_WG)
            a.hist_out[i] = a.hist_in[i + a.nsamp];
    __syncthreads();

    /* ---- one output per lane ---- */
    uint32_t clips = 0u;
    if (tid < outs) {
        int acc_i = 0, acc_q = 0;
        const uint2 *mine = fir_img + tid;
#pragma unroll 4
        for (int j = 0; j < a.npairs; j++) {
            const uint2 v = mine[a.off[j]]; /* slot tid + off_j < D * PL */
            const ds_s16x2 hp = __builtin_bit_cast(ds_s16x2, a.hp[j]);
            acc_i = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, v.x), hp, acc_i, false);
            acc_q = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, v.y), hp, acc_q, false);
        }
        const int yi = fir_round(acc_i, a.shift), yq = fir_round(acc_q, a.shift);
        const int ci = fir_clamp(yi), cq = fir_clamp(yq);
        clips = (uint32_t)(ci != yi) + (uint32_t)(cq != yq);
        a.out[m0 + tid] = ds_pair(ci, cq);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        clips += (uint32_t)__shfl_xor((int)clips, o);
    if (lane == 0 && clips)
        atomicAdd(a.clipped, (unsigned long long)clips);
}

} /* namespace gpsbb_impl */
#endif
