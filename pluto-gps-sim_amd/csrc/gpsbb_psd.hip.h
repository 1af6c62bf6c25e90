/*
 * gpsbb_psd.hip.h — k_psd, k_psd_fold: the power spectrum of gpsbb_device_psd (include/gpsbb.h has the definition in full; the
 * rules that need no GPU, the load, the twiddle product and the butterfly among them, are gpsbb_psd.h).  Hand-written HIP for
 * gfx950.  The definition fixes every value of the radix-2 transform, not where a value lies or when it is computed:
 *
 *   no bit reversal is ever done.  Sample n of a segment is point p = n, and the definition's a[bitrev(p)] is kept at p: the stage
 *       with h = 2^lh then pairs points that differ in bit q = log2n - 1 - lh of p, the first stage the top bit, the last bit 0, and
 *       its twiddle j * (4096 / m) is the 11-bit reversal of x = p >> (q + 1).  The table lies in LDS in that order (the host
 *       uploads it so), and a stage reads entry x: one entry for a whole wavefront in the early stages, consecutive entries for
 *       consecutive lanes in the late ones.  Only the even x are kept, twe[y] = entry 2 y: the reversal of 2 y + 1 is that of 2 y
 *       plus 1024, and the table's (c, s) there is (-s, c) of here by construction (psd_twiddles), so the odd entries are a swap and
 *       a negation away: 8 KiB of LDS at N = 4096 instead of 16, and one read less per unit.
 *       Bin k ends at point bitrev(k); k_psd_fold puts the sums in natural order.
 *   two stages per pass over LDS, in registers: a unit is the four points p0 + k e, k = 0..3, that differ in bits le + 1 and le
 *       (e = 2^le); stage one pairs (0, 2) and (1, 3) under entry t, stage two (0, 1) under entry 2 t and (2, 3) under
 *       entry 2 t + 1, t = p0 >> (le + 2).  Every step is the definition's radix-2 step with its own rounding (psd_tmul, psd_bfly).
 *       An odd log2n does its first stage, whose twiddle is (2^30, 0), while staging: t = v, no product.  The first pass's other
 *       exact twiddles, (2^30, 0) and (0, 2^30), are not multiplied either.
 *   a workgroup of four wavefronts holds M = max(N, 1024) points, 1024 / N segments at once for N < 1024, so that every lane has a
 *       unit in every pass; lane tid takes units tid + 256 r, r < M / 1024.
 *   the layout changes with every pass: for the pass with quarter stride e, point P lies at k (M / 4 + pad) + u with
 *       k = (P >> le) & 3 and u its unit.  A pass reads plane k at tid + 256 r: consecutive lanes, consecutive int2, one
 *       conflict-free ds_read_b64 per point whatever e is.  It writes its results where the NEXT pass reads them, so all reads of
 *       a pass are done (a barrier) before its writes begin.  In the natural layout the half-wave of a ds_read_b64 would hit
 *       8 of its 32 slots for e <= 8 and 16 for e = 16: 4-way and 2-way conflicts in the last three passes.
 *       The writes: the 16 lanes of a ds_write_b64 group (banks: 16 slots of 8 bytes) vary in u' % e', in the plane
 *       (u' / e') & 3 and above, e' = e / 4 the next pass's; pad = e' for e' < 16 makes the plane's bits land beside the lane's:
 *       16 distinct slots for every e', conflict-free.  The staging writes go to planes of e >= 16: consecutive.  (From the bank
 *       rule, not from a counter run)
 *   staged once per segment: the view (ds_view, the despreader's) of its N samples, windowed; lanes take consecutive samples.
 *   the sums: a lane keeps the uint64 of the 4 M / 1024 points it ends a transform with across its run of segments; at the end
 *       the segments a workgroup held side by side are added through LDS and one partial [N] per workgroup goes to scratch, which
 *       k_psd_fold adds.  No atomics; integer sums are order-free, the result does not depend on the launch's shape.
 *   segments past the run's end are staged as zeros: the transform of zeros is zero at every rounding, their power adds nothing.
 */
#ifndef GPSBB_PSD_HIP_H
#define GPSBB_PSD_HIP_H

#include "gpsbb_psd.h"
#include "gpsbb_despread.hip.h"

namespace gpsbb_impl {

constexpr int PSD_WG = 256;
constexpr int PSD_MIN_POINTS = 1024;   /* the points a workgroup holds at least: 1024 / N segments side by side for N < 1024 */
constexpr int PSD_RUN_BATCHES = 2;     /* a workgroup's run is at least this many loads of its LDS */
constexpr int PSD_MAX_WGS = 1024;      /* the grid's bound: partials of at most 1024 * 4096 * 8 bytes = 32 MiB */
constexpr int PSD_PAD = 8;             /* the largest pad between planes */
constexpr int PSD_MAX_UPL = GPSBB_PSD_MAX_N / 4 / PSD_WG; /* units per lane and pass at N = 4096 */

inline int psd_points(int log2n) { return (1 << log2n) > PSD_MIN_POINTS ? (1 << log2n) : PSD_MIN_POINTS; }
/* segments side by side in a workgroup, and the least run */
inline int psd_group(int log2n) { return psd_points(log2n) >> log2n; }
inline int psd_min_run(int log2n) { return psd_group(log2n) * PSD_RUN_BATCHES; }
/* bytes of LDS: four planes with their pads, then N / 4 twiddles */
inline size_t psd_lds_bytes(int log2n) { return ((size_t)psd_points(log2n) + 4 * PSD_PAD + ((size_t)1 << (log2n - 2))) * sizeof(psd_c); }
/* the run and the grid for nseg segments */
inline void psd_geometry(int log2n, long nseg, int *run, int *nwg)
{
    const long g = psd_group(log2n), r0 = psd_min_run(log2n);
    long w = (nseg + r0 - 1) / r0;
    w = w > PSD_MAX_WGS ? PSD_MAX_WGS : w;
    long r = (nseg + w - 1) / w;
    r = (r + g - 1) / g * g;
    *run = (int)r;
    *nwg = (int)((nseg + r - 1) / r);
}

struct PsdArgs {
    DsArgs d;                 /* iq, shift8, nz, ntab, it: what ds_view reads */
    const int32_t *tabs;      /* cos512[512], sin512[512] (INTERF) */
    const psd_c *tw;          /* [N / 4 at least] (c, s) of table index brev11(2 y) at y */
    const int16_t *win;       /* [N] */
    unsigned long long *part; /* [nwg][N], point order */
    long nseg, hop;
    int run, log2n, shift, wmul;
};

__device__ __forceinline__ int psd_pad(int le) { return le < 4 ? 1 << le : 0; }
/* where point P lies for the pass with quarter stride 2^le; Q = M / 4 */
__device__ __forceinline__ int psd_addr(int P, int le, int Q)
{
    const int k = (P >> le) & 3, u = ((P >> (le + 2)) << le) | (P & ((1 << le) - 1));
    return k * (Q + psd_pad(le)) + u;
}
/* v times the twiddle with table index 0 (odd false) or 1024 (odd true): v and -i v, exactly what psd_tmul gives for them */
__device__ __forceinline__ psd_c psd_exact(psd_c v, bool quarter) { return quarter ? psd_c{v.im, -v.re} : v; }

template <int VIEW, bool NOISE, bool INTERF>
__global__ __launch_bounds__(PSD_WG) void k_psd(PsdArgs a)
{
    extern __shared__ psd_c psd_lds[]; /* 4 (Q + PSD_PAD) points, N / 4 twiddles */
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint2 rep[INTERF ? 512 : 1]; /* .x = (cos, sin) as an int16 pair: ds_view's table */
    const int tid = (int)threadIdx.x;
    const int L = a.log2n, N = 1 << L, M = N > PSD_MIN_POINTS ? N : PSD_MIN_POINTS, Q = M >> 2, upl = Q / PSD_WG, G = M >> L;
    const bool odd = (L & 1) != 0;
    psd_c *dat = psd_lds, *twe = psd_lds + 4 * (Q + PSD_PAD);
    if (INTERF)
        for (int k = tid; k < 512; k += PSD_WG)
            rep[k] = make_uint2(ds_pair(a.tabs[k], a.tabs[512 + k]), 0u);
    if (NOISE)
        for (int k = tid; k < NOISE_KNOTS - 1; k += PSD_WG)
            ntab[k] = a.d.ntab[k];
    for (int k = tid; k < N / 4; k += PSD_WG)
        twe[k] = a.tw[k];
    const int le0 = L - (odd ? 3 : 2), npass = (L - (odd ? 1 : 0)) >> 1;
    unsigned long long acc[PSD_MAX_UPL][4];
#pragma unroll
    for (int r = 0; r < PSD_MAX_UPL; r++)
#pragma unroll
        for (int k = 0; k < 4; k++)
            acc[r][k] = 0ull;
    const long s_begin = (long)blockIdx.x * a.run, s_end = min(a.nseg, s_begin + (long)a.run); /* s_begin < nseg */

    for (long sb = s_begin; sb < s_end; sb += G) {
        __syncthreads(); /* the tables are there; the batch before has been read */
        /* ---- stage: the windowed view of G segments; an odd log2n takes its first stage (pairs N / 2 apart) on the way ---- */
        if (!odd) {
            for (int P = tid; P < M; P += PSD_WG) {
                const int n = P & (N - 1);
                const long sg = sb + (P >> L);
                psd_c x{0, 0};
                if (sg < s_end) {
                    const long i = sg * a.hop + n; /* < nsamp: segment sg < nseg lies inside the buffer */
                    const uint32_t w = ds_view<VIEW, NOISE, INTERF>(a.d.iq[i], (unsigned long long)i, a.d, ntab, rep);
                    const int wn = a.win[n];
                    x = psd_c{psd_load((int)(w << 16) >> 16, wn, a.wmul), psd_load((int)w >> 16, wn, a.wmul)};
                }
                dat[psd_addr(P, le0, Q)] = x;
            }
        } else {
            for (int it = tid; it < M / 2; it += PSD_WG) {
                const int n = it & (N / 2 - 1), g = it >> (L - 1), P = (g << L) | n;
                const long sg = sb + g;
                psd_c x0{0, 0}, x1{0, 0};
                if (sg < s_end) {
                    const long i0 = sg * a.hop + n, i1 = i0 + N / 2; /* < nsamp */
                    const uint32_t w0 = ds_view<VIEW, NOISE, INTERF>(a.d.iq[i0], (unsigned long long)i0, a.d, ntab, rep);
                    const uint32_t w1 = ds_view<VIEW, NOISE, INTERF>(a.d.iq[i1], (unsigned long long)i1, a.d, ntab, rep);
                    const int wn0 = a.win[n], wn1 = a.win[n + N / 2];
                    x0 = psd_c{psd_load((int)(w0 << 16) >> 16, wn0, a.wmul), psd_load((int)w0 >> 16, wn0, a.wmul)};
                    x1 = psd_c{psd_load((int)(w1 << 16) >> 16, wn1, a.wmul), psd_load((int)w1 >> 16, wn1, a.wmul)};
                    psd_bfly(x0, x1, x1);
                }
                dat[psd_addr(P, le0, Q)] = x0;
                dat[psd_addr(P + N / 2, le0, Q)] = x1;
            }
        }
        /* ---- the passes ---- */
        int le = le0;
        for (int ps = 0; ps < npass; ps++, le -= 2) {
            __syncthreads();
            psd_c v[PSD_MAX_UPL][4];
            const int plane = Q + psd_pad(le);
#pragma unroll
            for (int r = 0; r < PSD_MAX_UPL; r++)
                if (r < upl) {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        v[r][k] = dat[k * plane + tid + PSD_WG * r]; /* below 3 (Q + 8) + Q */
                }
            const bool last = ps == npass - 1;
            if (!last)
                __syncthreads(); /* every read of this pass before any write of it: the layouts differ */
#pragma unroll
            for (int r = 0; r < PSD_MAX_UPL; r++)
                if (r < upl) {
                    const int u = tid + PSD_WG * r, e = 1 << le;
                    const int p0 = ((u >> le) << (le + 2)) | (u & (e - 1)); /* < M */
                    const int t = (p0 & (N - 1)) >> (le + 2);               /* < N / 4 */
                    psd_c t0, t1;
                    if (ps == 0) { /* t is 0, or 0 or 1 behind the staged stage: (2^30, 0) and (0, 2^30) */
                        t0 = psd_exact(v[r][2], t != 0);
                        t1 = psd_exact(v[r][3], t != 0);
                    } else {
                        psd_c w = twe[t >> 1];
                        w = (t & 1) ? psd_c{-w.im, w.re} : w;
                        t0 = psd_tmul(v[r][2], w.re, w.im);
                        t1 = psd_tmul(v[r][3], w.re, w.im);
                    }
                    psd_bfly(v[r][0], v[r][2], t0);
                    psd_bfly(v[r][1], v[r][3], t1);
                    if (ps == 0 && !odd) { /* t = 0: table indices 0 and 1024 */
                        t0 = v[r][1];
                        t1 = psd_exact(v[r][3], true);
                    } else {
                        const psd_c wa = twe[t];
                        t0 = psd_tmul(v[r][1], wa.re, wa.im);
                        t1 = psd_tmul(v[r][3], -wa.im, wa.re);
                    }
                    psd_bfly(v[r][0], v[r][1], t0);
                    psd_bfly(v[r][2], v[r][3], t1);
                    if (last) { /* le == 0: points 4 u + k */
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            acc[r][k] += psd_power(v[r][k], a.shift);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            dat[psd_addr(p0 + k * e, le - 2, Q)] = v[r][k];
                    }
                }
        }
    }
    /* ---- the segments held side by side, added: point P = 4 u + k of the last pass holds bin bitrev(P mod N) of segment P / N ---- */
    __syncthreads();
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(dat); /* [M] */
#pragma unroll
    for (int r = 0; r < PSD_MAX_UPL; r++)
        if (r < upl) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                sums[4 * (tid + PSD_WG * r) + k] = acc[r][k];
        }
    __syncthreads();
    for (int p = tid; p < N; p += PSD_WG) {
        unsigned long long s = 0ull;
        for (int g = 0; g < G; g++)
            s += sums[(g << L) + p];
        a.part[(size_t)blockIdx.x * (size_t)N + (size_t)p] = s;
    }
}

/* psd[bitrev(p)] = the sum over the workgroups' partials of point p.  A block takes 32 points; its eight slices of 32 lanes take
 * every eighth partial each (rows of 256 bytes, loads that do not wait for one another) and are added through LDS: with one lane
 * per point the 1024 partials of a large call were 1024 loads in a row: 0.18 of the 0.22 ms of 2 500 000 samples at N = 256. */
constexpr int PSD_FOLD_BINS = 32, PSD_FOLD_SLICES = 8;
__global__ __launch_bounds__(PSD_FOLD_BINS * PSD_FOLD_SLICES) void k_psd_fold(const unsigned long long *__restrict__ part, unsigned long long *__restrict__ psd,
                                                                            int log2n, int nwg)
{
    __shared__ unsigned long long red[PSD_FOLD_SLICES][PSD_FOLD_BINS];
    const int N = 1 << log2n, b = (int)threadIdx.x % PSD_FOLD_BINS, sl = (int)threadIdx.x / PSD_FOLD_BINS;
    const int p = (int)blockIdx.x * PSD_FOLD_BINS + b; /* < N: the grid is N / 32 blocks, N >= 64 */
    unsigned long long s = 0ull;
#pragma unroll 4
    for (int w = sl; w < nwg; w += PSD_FOLD_SLICES)
        s += part[(size_t)w * (size_t)N + (size_t)p];
    red[sl][b] = s;
    __syncthreads();
    if (sl == 0) {
#pragma unroll
        for (int k = 1; k < PSD_FOLD_SLICES; k++)
            s += red[k][b];
        psd[__brev((unsigned)p) >> (32 - log2n)] = s;
    }
}

} /* namespace gpsbb_impl */
#endif
