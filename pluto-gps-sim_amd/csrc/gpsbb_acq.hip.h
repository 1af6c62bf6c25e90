/*
 * gpsbb_acq.hip.h — k_acq: the blind search of gpsbb_device_acquire (include/gpsbb.h has the definition in full; the host-side
 * rules are gpsbb_acq.h).  Hand-written HIP for gfx950, and the first kernel here that is shaped like a matrix product: for one
 * Doppler bin, S(p, L) = sum over m of X[p][m] * Y[m + L] is the 32 codes (+-1 as int8) times a Hankel matrix of the mixed
 * signal, and 32 codes x 32 delays x 32 samples are one v_mfma_i32_32x32x32_i8.
 *
 *   digits: yI and yQ are split into D signed base-256 digits d_j in [-128, 127] (SC16: |y| < 2^25, D = 4; SC8: 2^17, 3; SC1: 2).
 *       Each digit plane is one MFMA per K-step; its int32 accumulator is exact (a plane's sum stays below 128 * N <= 2^27) and
 *       the planes are put together in int64 at the end of an interval: S = sum of acc_j * 256^j.
 *   a workgroup (four wavefronts) takes one bin and four consecutive delay tiles of 32, one tile per wavefront.  Per chunk of
 *       AQ_KC replica samples it stages the view (ds_view, the despreader's) of the AQ_KC + 128 samples its tiles look at ONCE,
 *       mixes each once, and writes the digits to LDS.  A position at or beyond nsamp is staged as zero and never read.
 *   the B fragment of lane l = (g, r) is 16 consecutive digit bytes from byte offset m0 + 16 g + 32 wave + r — any alignment — so
 *       every plane is kept four times, copy s moved s bytes down: the fragment is four aligned dwords of copy (offset & 3).
 *   the A fragment depends on the replica sample only: k_acq_chips expands the chips of the 32 PRNs once per call into
 *       int8 [nnc][32][npad] (npad = N rounded up to 32), zero for a PRN outside the mask and for m >= N, so a K-step never
 *       crosses an interval and the ragged last step adds nothing.  Lane (g, r) reads 16 aligned bytes of row r.
 *   lane map: A and B of one lane sit at the same k by construction (both are "bytes 16 g .. 16 g + 15 of the step"), so only the
 *       C/D map matters: column (delay) = lane & 31, row (PRN) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
 *   no floating point and no atomics: a tile writes its M to the grid where wanted and one partial (max, smallest lag, 128-bit
 *       sum) per (PRN, bin, tile); k_acq_fold folds the partials in tile order into the rows.
 */
#ifndef GPSBB_ACQ_HIP_H
#define GPSBB_ACQ_HIP_H

#include "gpsbb_acq.h"
#include "gpsbb_despread.hip.h"

namespace gpsbb_impl {

constexpr int AQ_WG = 256;
constexpr int AQ_WAVES = AQ_WG / 64;
constexpr int AQ_KC = 256;                /* replica samples per staged chunk */
constexpr int AQ_LT = 32 * AQ_WAVES;      /* delays per workgroup */
constexpr int AQ_SPAN = AQ_KC + AQ_LT;    /* samples staged per chunk */
constexpr int AQ_STRIDE = AQ_SPAN + 16;   /* bytes per plane copy */
static_assert(AQ_KC % 32 == 0 && AQ_STRIDE % 4 == 0, "whole K-steps, dword rows");

typedef int aq_i32x4 __attribute__((ext_vector_type(4)));
typedef int aq_i32x16 __attribute__((ext_vector_type(16)));

struct AcqArgs {
    DsArgs d;                  /* iq, shift8, nz, ntab, it: what ds_view reads */
    const int32_t *tabs;       /* cos512[512], sin512[512] */
    const int8_t *chips;       /* [nnc][32][npad] */
    unsigned long long *grid;  /* [32][nbins][nlags] or nullptr */
    gpsbb_acq_row_t *part;     /* [32][nbins][ntiles] */
    long nsamp;
    int nbins, ncoh, npad, nlags, nnc, shift, ntiles;
    int step[GPSBB_ACQ_MAX_BINS];
};

constexpr int aq_digits(int view) { return view == DS_SC16 ? 4 : (view == PACK_SC8 ? 3 : 2); }

/* out[i][p][m] = +-1, the chip of PRN p + 1 at replica sample i * ncoh + m; 0 outside the mask and for m >= ncoh */
__global__ __launch_bounds__(256) void k_acq_chips(const uint32_t *__restrict__ ca_bits, int8_t *__restrict__ out, uint32_t mask,
                                                   unsigned long long code_step, int ncoh, int npad, int nnc)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)nnc * npad)
        return;
    const int i = (int)(q / npad), m = (int)(q % npad);
    const bool in = m < ncoh;
    const uint32_t c = (uint32_t)(((code_step * (unsigned long long)((long long)i * ncoh + m)) >> 32) % (unsigned long long)GPSBB_CA_LEN);
    for (int p = 0; p < ACQ_PRNS; p++) {
        const uint32_t bit = (ca_bits[(p + 1) * 32 + (c >> 5)] >> (c & 31u)) & 1u;
        out[((size_t)i * ACQ_PRNS + p) * (size_t)npad + m] = (int8_t)(in && ((mask >> p) & 1u) ? (bit ? 1 : -1) : 0);
    }
}

template <int VIEW, bool NOISE, bool INTERF>
__global__ __launch_bounds__(AQ_WG) void k_acq(AcqArgs a)
{
    constexpr int D = aq_digits(VIEW);
    __shared__ uint2 rep[512]; /* .x = (cos, sin) as an int16 pair: ds_view's table and the mixer's */
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ __attribute__((aligned(16))) uint8_t planes[2][D][4][AQ_STRIDE]; /* [I/Q][digit][copy s][byte b] = digit of sample b + s */
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 5, r = lane & 31;
    const int bin = (int)blockIdx.y;
    const int tile = (int)blockIdx.x * AQ_WAVES + wave;
    const int lbase = (int)blockIdx.x * AQ_LT;
    const bool live = tile < a.ntiles; /* (uniform over the wavefront) */
    for (int k = tid; k < 512; k += AQ_WG)
        rep[k] = make_uint2(ds_pair(a.tabs[k], a.tabs[512 + k]), 0u);
    if (NOISE)
        for (int k = tid; k < NOISE_KNOTS - 1; k += AQ_WG)
            ntab[k] = a.d.ntab[k];
    const uint32_t step = (uint32_t)a.step[bin];
    unsigned long long M[16];
#pragma unroll
    for (int q = 0; q < 16; q++)
        M[q] = 0ull;
    for (int i = 0; i < a.nnc; i++) {
        aq_i32x16 acc[2][D];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int j = 0; j < D; j++)
#pragma unroll
                for (int q = 0; q < 16; q++)
                    acc[c][j][q] = 0;
        for (int ms = 0; ms < a.ncoh; ms += AQ_KC) {
            __syncthreads(); /* the tables are there; the last chunk's fragments have been read */
            /* ---- stage: view and mix of samples i N + ms + lbase + t, once each, as digit bytes in four copies ---- */
            for (int t = tid; t < AQ_SPAN; t += AQ_WG) {
                const long n = (long)i * a.ncoh + ms + lbase + t;
                int y[2] = {0, 0};
                if (n < a.nsamp) {
                    const uint32_t w = ds_view<VIEW, NOISE, INTERF>(a.d.iq[n], (unsigned long long)n, a.d, ntab, rep);
                    const int wi = (int)(w << 16) >> 16, wq = (int)w >> 16;
                    const uint32_t cs = rep[(step * (uint32_t)n) >> 23].x;
                    const int c = (int)(cs << 16) >> 16, s = (int)cs >> 16;
                    y[0] = wi * c + wq * s;
                    y[1] = wq * c - wi * s;
                }
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    int v = y[c];
#pragma unroll
                    for (int j = 0; j < D; j++) {
                        const int dg = (int)(int8_t)(v & 0xff);
                        v = (v - dg) >> 8;
#pragma unroll
                        for (int s = 0; s < 4; s++)
                            if (t >= s)
                                planes[c][j][s][t - s] = (uint8_t)dg;
                    }
                }
            }
            __syncthreads();
            if (live) {
                const int kend = min(AQ_KC, a.npad - ms);
                const int8_t *__restrict__ arow = a.chips + ((size_t)i * ACQ_PRNS + r) * (size_t)a.npad + ms + 16 * g;
                for (int m0 = 0; m0 < kend; m0 += 32) {
                    const aq_i32x4 av = *reinterpret_cast<const aq_i32x4 *>(arow + m0);
                    const int o = m0 + 16 * g + 32 * wave + r;
                    const int s = o & 3, ab = o & ~3;
#pragma unroll
                    for (int c = 0; c < 2; c++)
#pragma unroll
                        for (int j = 0; j < D; j++) {
                            const uint32_t *pp = reinterpret_cast<const uint32_t *>(&planes[c][j][s][ab]);
                            aq_i32x4 bv;
                            bv[0] = (int)pp[0];
                            bv[1] = (int)pp[1];
                            bv[2] = (int)pp[2];
                            bv[3] = (int)pp[3];
                            acc[c][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc[c][j], 0, 0, 0);
                        }
                }
            }
        }
        /* ---- the interval's sums, exact in int64, into the metric ---- */
#pragma unroll
        for (int q = 0; q < 16; q++) {
            long long S[2] = {0, 0};
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int j = 0; j < D; j++)
                    S[c] += (long long)acc[c][j][q] * (1ll << (8 * j));
            const unsigned long long ui = (unsigned long long)(S[0] >> a.shift), uq = (unsigned long long)(S[1] >> a.shift);
            M[q] += ui * ui + uq * uq;
        }
    }
    if (!live)
        return;
    /* ---- out: column (delay) = lane & 31, row (PRN - 1) = (q & 3) + 8 (q >> 2) + 4 (lane >> 5) ---- */
    const int L = tile * 32 + r;
    const bool has = L < a.nlags;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int p = (q & 3) + 8 * (q >> 2) + 4 * g;
        if (a.grid && has)
            a.grid[((size_t)p * a.nbins + bin) * (size_t)a.nlags + L] = M[q];
        unsigned long long peak = has ? M[q] : 0ull, lo = peak, hi = 0ull;
        int lag = has ? L : 0x7fffffff;
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) { /* (within the lane's half: the other half holds other PRNs) */
            const unsigned long long op = __shfl_xor(peak, off), ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
            const int og = __shfl_xor(lag, off);
            const bool take = op > peak || (op == peak && og < lag);
            peak = take ? op : peak;
            lag = take ? og : lag;
            lo += ol;
            hi += oh + (lo < ol ? 1ull : 0ull);
        }
        if (r == 0) {
            gpsbb_acq_row_t o;
            o.peak = peak;
            o.sum_lo = lo;
            o.sum_hi = hi;
            o.lag = lag;
            o._pad = 0;
            a.part[((size_t)p * a.nbins + bin) * (size_t)a.ntiles + tile] = o;
        }
    }
}

/* rows[q] of (PRN, bin) q from its ntiles partials, in tile order: the first tile that attains the peak holds the smallest lag */
__global__ __launch_bounds__(256) void k_acq_fold(const gpsbb_acq_row_t *__restrict__ part, gpsbb_acq_row_t *__restrict__ rows, int nrows,
                                                  int ntiles)
{
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= nrows)
        return;
    gpsbb_acq_row_t o = part[(size_t)q * ntiles];
    for (int t = 1; t < ntiles; t++) {
        const gpsbb_acq_row_t x = part[(size_t)q * ntiles + t];
        if (x.peak > o.peak) {
            o.peak = x.peak;
            o.lag = x.lag;
        }
        o.sum_lo += x.sum_lo;
        o.sum_hi += x.sum_hi + (o.sum_lo < x.sum_lo ? 1ull : 0ull);
    }
    rows[q] = o;
}

} /* namespace gpsbb_impl */
#endif
