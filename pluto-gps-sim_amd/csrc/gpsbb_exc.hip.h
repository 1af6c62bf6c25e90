/*
 * gpsbb_exc.hip.h — k_excise, k_exc_fold: the interference excision of gpsbb_device_excise (include/gpsbb.h has the definition in
 * full; the rules that need no GPU, the decision, the reduce step, the inverse's product and butterfly and the overlap-add among
 * them, are gpsbb_exc.h).  Hand-written HIP for gfx950.  A segment goes from the view to the output without leaving LDS:
 *
 *   forward: k_psd's transform as it stands there (gpsbb_psd.hip.h: no bit reversal, two stages per LDS pass in registers, the
 *       layout moving with the pass, the table in reversed order), repeated here and not shared so that k_psd's code does not
 *       change.  It ends with the four points 4 u + k of a unit in a lane's registers, bin k at point bitrev(k).
 *   decide and reduce there, in registers: the host uploads the mask in point order, a unit's four bits are one nibble.
 *   inverse: point bitrev(k) is exactly where the definition's a[] has Z[k], so the inverse pairs bit 0 of the point first and ends
 *       with sample n at point n: no bit reversal anywhere.  Its first two stages pair the four points a lane holds, under the
 *       exact twiddles (2^30, 0) and (0, 2^30): no product, no LDS.  Every further pass reads a unit p0 + k e, k = 0..3
 *       (e = 2^le, le = 2, 4, ..), does the stage with h = e on (0, 1) and (2, 3) and the stage with h = 2 e on (0, 2) and (1, 3),
 *       and writes where the next pass reads.  The twiddles j * (4096 / m) are wanted in natural order here, j = u mod e: a second
 *       arrangement of the table, per pass one entry (c, s of the stage h = e; c, s of the stage h = 2 e at j) per j — the entry
 *       at j + e is (-s, c) of the one at j by construction (psd_twiddles) — read by consecutive lanes as consecutive 16 bytes.
 *       An odd log2n has one stage left, h = N / 2: a pass of its own over pairs n, n + N / 2 in place.
 *   layouts: psd_addr's planes with the inverse's own pads.  A pass reads plane k at tid + 256 r: consecutive lanes, consecutive
 *       int2, one conflict-free ds_read_b64 per point.  The 16 lanes of a ds_write_b64 group (16 slots of 8 bytes) write, for the
 *       pass after e = 1, plane u % 4 at 4 (u / 4) + k: pad 1 puts the plane's two bits beside the unit's, 16 distinct slots; after
 *       e = 4, plane (u / 4) % 4 at 16 (u / 16) + 4 k + u % 4: pad 4 does the same; from e = 16 on, and into the natural order the
 *       last pass leaves, the group's lanes are consecutive.  (From the bank rule, not from a counter run)
 *   overlap-add: the batch's y lie in natural order; block s - 1 is the second half of segment s - 1 — the segment to the left in
 *       the batch, or the carry, the second half the batch before left in LDS — plus the first half of segment s, shifted, clamped
 *       and stored as one int16 pair per lane, consecutive lanes consecutive samples.
 *   a workgroup takes a run of consecutive blocks [b0, b1) and so the segments b0 .. b1: its first segment only seeds the carry
 *       (the workgroup before owns its block and its count), one segment per run is computed twice.  M = max(N, 1024) points are
 *       held at once, 1024 / N segments side by side for N < 1024, as in k_psd.
 *   staged once per sample and segment: ds_view (SC16) of the sample, or the uploaded history before sample 0; the last segment,
 *       the last N of hist_in ++ w, is also written out as the history to hand on.
 *   no atomics: a lane counts what it zeroed and what its clamp changed, the workgroup adds them through LDS, k_exc_fold adds the
 *       workgroups'.  Integer sums are order-free: the result does not depend on the launch's shape.
 */
#ifndef GPSBB_EXC_HIP_H
#define GPSBB_EXC_HIP_H

#include "gpsbb_exc.h"
#include "gpsbb_psd.hip.h"

namespace gpsbb_impl {

constexpr int EXC_RUN_BATCHES = 4; /* a workgroup's run is at least this many loads of its LDS, less the one block it recomputes */
constexpr int EXC_MAX_WGS = 1024;  /* the grid's bound: longer runs beyond it */

struct alignas(16) exc_tw {
    int32_t c1, s1, c2, s2; /* the stage h = e at j, the stage h = 2 e at j */
};

/* entries of the passes' table: e of them for le = 2, 4, .. while le + 2 <= log2n; the pass le begins at (e - 4) / 3 */
inline int exc_tw_entries(int log2n)
{
    int n = 0;
    for (int le = 2; le + 2 <= log2n; le += 2)
        n += 1 << le;
    return n;
}
/* entries of the last stage's table: N / 2 for an odd log2n */
inline int exc_fin_entries(int log2n) { return (log2n & 1) ? 1 << (log2n - 1) : 0; }
/* 8-byte words of one log2n's tables in device memory, and where they begin (log2n 6 first) */
inline size_t exc_tab_words(int log2n) { return 2 * (size_t)exc_tw_entries(log2n) + (size_t)exc_fin_entries(log2n); }
inline size_t exc_tab_offset(int log2n)
{
    size_t o = 0;
    for (int l = EXC_MIN_LOG2N; l < log2n; l++)
        o += exc_tab_words(l);
    return o;
}
/* the tables as k_excise reads them: the passes' entries, then the last stage's */
inline void exc_tables(int log2n, const int32_t *c, const int32_t *s, exc_tw *tw, psd_c *fin)
{
    for (int le = 2; le + 2 <= log2n; le += 2)
        for (int j = 0; j < (1 << le); j++) {
            const int k1 = j * (2048 >> le), k2 = j * (1024 >> le);
            *tw++ = exc_tw{c[k1], s[k1], c[k2], s[k2]};
        }
    for (int n = 0; n < exc_fin_entries(log2n); n++)
        fin[n] = psd_c{c[n * (4096 >> log2n)], s[n * (4096 >> log2n)]};
}
/* mask bit of point p: bin bitrev(p) */
inline void exc_mask_points(const gpsbb_exc_t *e, uint32_t *mp /* [N / 32] */)
{
    const int L = e->log2n, N = 1 << L;
    for (int i = 0; i < N / 32; i++)
        mp[i] = 0;
    for (int k = 0; k < N; k++)
        if (exc_masked(e, k)) {
            uint32_t p = 0;
            for (int b = 0; b < L; b++)
                p |= (((uint32_t)k >> b) & 1u) << (L - 1 - b);
            mp[p >> 5] |= 1u << (p & 31);
        }
}

/* segments side by side, the least run in blocks, LDS */
inline int exc_min_run(int log2n) { return psd_group(log2n) * EXC_RUN_BATCHES - 1; }
inline size_t exc_lds_bytes(int log2n)
{
    const size_t N = (size_t)1 << log2n;
    return ((size_t)psd_points(log2n) + 4 * PSD_PAD + N / 4 + N / 2 + (size_t)exc_fin_entries(log2n)) * sizeof(psd_c) +
           (size_t)exc_tw_entries(log2n) * sizeof(exc_tw) + N / 8;
}
/* the run (blocks per workgroup: run + 1 segments, a multiple of the group) and the grid for nblk blocks */
inline void exc_geometry(int log2n, long nblk, int *run, int *nwg)
{
    const long g = psd_group(log2n), r0 = exc_min_run(log2n);
    long w = (nblk + r0 - 1) / r0;
    w = w > EXC_MAX_WGS ? EXC_MAX_WGS : w;
    long r = (nblk + w - 1) / w;
    r = (r + 1 + g - 1) / g * g - 1;
    *run = (int)r;
    *nwg = (int)((nblk + r - 1) / r);
}

struct ExcArgs {
    DsArgs d;                 /* iq, nz, ntab, it: what ds_view reads */
    const int32_t *tabs;      /* cos512[512], sin512[512] (INTERF) */
    const psd_c *tw;          /* k_psd's table */
    const exc_tw *itw;        /* [exc_tw_entries] */
    const psd_c *fin;         /* [exc_fin_entries] */
    const int16_t *win;       /* [N] */
    const uint32_t *maskp;    /* [N / 32] the mask in point order */
    const uint32_t *hist_in;  /* [N] samples (Q << 16 | I) */
    uint32_t *hist_out;       /* [N] */
    uint32_t *out;            /* [nsamp] */
    unsigned long long *part; /* [nwg][2]: clipped, excised */
    unsigned long long thr;
    long nblk;
    int run, log2n;
};

__device__ __forceinline__ int exc_pad(int le) { return le == 2 ? 1 : (le == 4 ? 4 : 0); }
/* where point P lies for the inverse's pass with quarter stride 2^le; Q = M / 4 */
__device__ __forceinline__ int exc_addr(int P, int le, int Q)
{
    const int k = (P >> le) & 3, u = ((P >> (le + 2)) << le) | (P & ((1 << le) - 1));
    return k * (Q + exc_pad(le)) + u;
}

template <bool NOISE, bool INTERF>
__global__ __launch_bounds__(PSD_WG) void k_excise(ExcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) psd_c exc_lds[]; /* 4 (Q + PSD_PAD) points, N / 4 twiddles, N / 2 carry, the last stage's, the passes', the mask */
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    __shared__ uint2 rep[INTERF ? 512 : 1]; /* .x = (cos, sin) as an int16 pair: ds_view's table */
    __shared__ unsigned long long red[2][PSD_WG / 64];
    const int tid = (int)threadIdx.x;
    const int L = a.log2n, N = 1 << L, H = N >> 1, M = N > PSD_MIN_POINTS ? N : PSD_MIN_POINTS, Q = M >> 2, upl = Q / PSD_WG, G = M >> L;
    const int RG = exc_g(L), S = 13 - RG;
    const bool odd = (L & 1) != 0;
    const int nfin = odd ? H : 0, ntw = ((1 << (L & ~1)) - 4) / 3; /* exc_fin_entries, exc_tw_entries */
    psd_c *dat = exc_lds, *twe = dat + 4 * (Q + PSD_PAD), *carry = twe + N / 4, *fin = carry + H;
    exc_tw *itw = reinterpret_cast<exc_tw *>(fin + nfin); /* 16-byte aligned: every count before it is even */
    uint32_t *maskp = reinterpret_cast<uint32_t *>(itw + ntw);
    if (INTERF)
        for (int k = tid; k < 512; k += PSD_WG)
            rep[k] = make_uint2(ds_pair(a.tabs[k], a.tabs[512 + k]), 0u);
    if (NOISE)
        for (int k = tid; k < NOISE_KNOTS - 1; k += PSD_WG)
            ntab[k] = a.d.ntab[k];
    for (int k = tid; k < N / 4; k += PSD_WG)
        twe[k] = a.tw[k];
    for (int k = tid; k < ntw; k += PSD_WG)
        itw[k] = a.itw[k];
    for (int k = tid; k < nfin; k += PSD_WG)
        fin[k] = a.fin[k];
    for (int k = tid; k < N / 32; k += PSD_WG)
        maskp[k] = a.maskp[k];
    const int le0 = L - (odd ? 3 : 2), npass = (L - (odd ? 1 : 0)) >> 1;
    const long b0 = (long)blockIdx.x * a.run, b1 = min(a.nblk, b0 + (long)a.run); /* blocks [b0, b1), segments b0 .. b1; b0 < nblk */
    uint32_t clips = 0, nexc = 0;

    for (long sb = b0; sb <= b1; sb += G) {
        __syncthreads(); /* the tables are there; the batch before has been read */
        /* ---- stage: the windowed samples of G segments; an odd log2n takes its first stage (pairs N / 2 apart) on the way ---- */
        for (int it = tid; it < (odd ? M / 2 : M); it += PSD_WG) {
            const int n = odd ? it & (H - 1) : it & (N - 1), g = odd ? it >> (L - 1) : it >> L, P = (g << L) | n;
            const long sg = sb + g;
            psd_c x0{0, 0}, x1{0, 0};
            if (sg <= b1) {
#pragma unroll
                for (int hf = 0; hf < 2; hf++)
                    if (hf == 0 || odd) {
                        const int m = n + hf * H;
                        const long i = (sg - 2) * (long)H + m; /* in [-N, nsamp): sg <= nblk */
                        uint32_t w;
                        if (i >= 0)
                            w = ds_view<DS_SC16, NOISE, INTERF>(a.d.iq[i], (unsigned long long)i, a.d, ntab, rep);
                        else
                            w = a.hist_in[i + N];
                        if (sg == a.nblk)
                            a.hist_out[m] = w; /* the last segment is the last N of hist_in ++ w */
                        const int wn = a.win[m];
                        const psd_c x{psd_load((int)(w << 16) >> 16, wn, 1), psd_load((int)w >> 16, wn, 1)};
                        if (hf == 0)
                            x0 = x;
                        else
                            x1 = x;
                    }
                if (odd)
                    psd_bfly(x0, x1, x1);
            }
            dat[psd_addr(P, le0, Q)] = x0;
            if (odd)
                dat[psd_addr(P + H, le0, Q)] = x1;
        }
        /* ---- the forward passes: k_psd's ---- */
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
                    if (!last) {
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            dat[psd_addr(p0 + k * e, le - 2, Q)] = v[r][k];
                    } else { /* le == 0: points 4 u + k hold X[bitrev]: decide, reduce, and the inverse's stages h = 1 and h = 2 */
                        const int pn = p0 & (N - 1);
                        const uint32_t bits = maskp[pn >> 5] >> (pn & 31);
                        const long sg = sb + (p0 >> L);
                        const bool counted = sg > b0 && sg <= b1;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const bool z = exc_zeroed(v[r][k], (bits >> k) & 1u, a.thr);
                            nexc += z && counted;
                            v[r][k] = z ? psd_c{0, 0} : exc_reduce(v[r][k], RG);
                        }
                        exc_bfly(v[r][0], v[r][1], v[r][1]);
                        exc_bfly(v[r][2], v[r][3], v[r][3]);
                        exc_bfly(v[r][0], v[r][2], v[r][2]);
                        exc_bfly(v[r][1], v[r][3], psd_c{-v[r][3].im, v[r][3].re}); /* table index 1024: (0, 2^30), t = i v */
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            dat[exc_addr(p0 + k, 2, Q)] = v[r][k];
                    }
                }
        }
        /* ---- the inverse's passes: stages h = e and h = 2 e ---- */
        for (le = 2; le + 2 <= L; le += 2) {
            __syncthreads();
            psd_c v[PSD_MAX_UPL][4];
            const int plane = Q + exc_pad(le);
#pragma unroll
            for (int r = 0; r < PSD_MAX_UPL; r++)
                if (r < upl) {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        v[r][k] = dat[k * plane + tid + PSD_WG * r];
                }
            const bool natural = le + 4 > L; /* no pass of two stages follows */
            __syncthreads();
#pragma unroll
            for (int r = 0; r < PSD_MAX_UPL; r++)
                if (r < upl) {
                    const int u = tid + PSD_WG * r, e = 1 << le, j = u & (e - 1);
                    const int p0 = ((u >> le) << (le + 2)) | j; /* < M */
                    const exc_tw w = itw[(e - 4) / 3 + j];
                    exc_bfly(v[r][0], v[r][1], exc_tmul(v[r][1], w.c1, w.s1));
                    exc_bfly(v[r][2], v[r][3], exc_tmul(v[r][3], w.c1, w.s1));
                    exc_bfly(v[r][0], v[r][2], exc_tmul(v[r][2], w.c2, w.s2));
                    exc_bfly(v[r][1], v[r][3], exc_tmul(v[r][3], -w.s2, w.c2)); /* j + e: index + 1024 */
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        dat[natural ? p0 + k * e : exc_addr(p0 + k * e, le + 2, Q)] = v[r][k];
                }
        }
        __syncthreads();
        if (odd) { /* the stage h = N / 2, in place: a lane reads and writes its own pair */
            for (int it = tid; it < M / 2; it += PSD_WG) {
                const int n = it & (H - 1), P = ((it >> (L - 1)) << L) | n;
                psd_c x0 = dat[P], x1 = dat[P + H];
                const psd_c w = fin[n];
                exc_bfly(x0, x1, exc_tmul(x1, w.re, w.im));
                dat[P] = x0;
                dat[P + H] = x1;
            }
            __syncthreads();
        }
        /* ---- overlap-add: block sg - 1 from the second half to the left and the first half of segment sg ---- */
        for (int it = tid; it < M / 2; it += PSD_WG) {
            const int n = it & (H - 1), g = it >> (L - 1);
            const long sg = sb + g;
            if (sg > b0 && sg <= b1) {
                const psd_c p = g ? dat[((g - 1) << L) + H + n] : carry[n], c = dat[(g << L) + n];
                const int32_t oi = exc_ola(p.re, c.re, S, clips), oq = exc_ola(p.im, c.im, S, clips);
                a.out[(sg - 1) * (long)H + n] = ((uint32_t)oi & 0xffffu) | ((uint32_t)oq << 16); /* below nblk * H = nsamp */
            }
        }
        __syncthreads();
        for (int n = tid; n < H; n += PSD_WG)
            carry[n] = dat[((G - 1) << L) + H + n];
    }
    /* ---- the counts ---- */
    unsigned long long c0 = clips, c1 = nexc;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        c0 += (unsigned long long)__shfl_xor((int)(uint32_t)c0, o) & 0xffffffffull;
        c1 += (unsigned long long)__shfl_xor((int)(uint32_t)c1, o) & 0xffffffffull;
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = c0;
        red[1][tid >> 6] = c1;
    }
    __syncthreads();
    if (tid < 2) {
        unsigned long long s = 0ull;
        for (int k = 0; k < PSD_WG / 64; k++)
            s += red[tid][k];
        a.part[2 * (size_t)blockIdx.x + (size_t)tid] = s;
    }
}

/* out[0], out[1] = the sums of the workgroups' counts */
__global__ __launch_bounds__(PSD_WG) void k_exc_fold(const unsigned long long *__restrict__ part, unsigned long long *__restrict__ out, int nwg)
{
    __shared__ unsigned long long red[2][PSD_WG];
    const int tid = (int)threadIdx.x;
    unsigned long long s0 = 0ull, s1 = 0ull;
    for (int w = tid; w < nwg; w += PSD_WG) {
        s0 += part[2 * (size_t)w];
        s1 += part[2 * (size_t)w + 1];
    }
    red[0][tid] = s0;
    red[1][tid] = s1;
    __syncthreads();
    for (int o = PSD_WG / 2; o; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
        }
        __syncthreads();
    }
    if (tid < 2)
        out[tid] = red[tid][0];
}

} /* namespace gpsbb_impl */
#endif
