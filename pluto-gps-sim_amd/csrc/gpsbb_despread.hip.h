/*
 * gpsbb_despread.hip.h — k_despread: the synthesis turned round.  Rendered IQ in device memory is correlated with every
 * channel's own replica — dataBit * codeCA * (cosTable512[iTable], sinTable512[iTable]) exactly as the reference's loop holds
 * them at that sample (c:2697-2737) — into one prompt sum per channel and segment (include/gpsbb.h: gpsbb_batch_despread has
 * the definition in full).  Hand-written HIP for gfx950.
 *
 * The replica is not tracked, it is KNOWN: a batch that has run leaves the exact NCO state of every channel at every tile
 * (or granule of tiles) in tile_x / tile_nav, and index and chip of a sample follow from them the way k_synth_pd gets them:
 *
 *   lane = sample mod 64.  A lane loads its 16 samples of a tile ONCE (256 contiguous bytes per wavefront and load), applies
 *       noise and quantiser once, and keeps the 16 (uI, uQ) pairs in registers across the channel loop: 4 bytes read per
 *       sample, whatever the channel count.  The 64 lanes look at 64 consecutive samples, so the table reads below are
 *       consecutive or equal addresses (conflict-free, chips mostly a broadcast).
 *   the model in guard format, per sample: fma(n, step, 2^20 + W + state) with n counted from the state's own sample (the
 *       tile's first, or the first of the tile's granule: BatchDev::st_log2).  One unit in the last place is 2^-32, the low
 *       word IS the fraction, the low bits of the high word ARE index and chip.  Against the truth the model is off by the
 *       roundings of at most 4095 additions of the reference's recurrence (each within half an ulp of a number below
 *       2048 chips: 2^-43, i.e. 2^-11 units) — 2.5 units for a granule of four tiles, 0.5 for a tile — plus the state put
 *       into guard format and the fma, half a unit each: under 4 units, against the bias W = PD_BAND = 20 (k_synth_pd's
 *       budget, kept: its additions pile up roundings that an fma per sample does not).  floor(model) = floor(truth)
 *       unless the model's low word is below 2W; such a sample (DsArgs::danger) takes index, chip and data bit from the
 *       exact jump-ahead (gpsbb_nco.h) from the same state, as pd_fix_sample does.  Exact unconditionally.
 *   a falling carrier is walked mirrored (512 - phase, |step|) and its index mirrored back (^ 511): see ev_first.
 *   the replica table is the carrier table itself, at gain 1.0 — ONE table for all channels: per index the int16 pairs
 *       (cos, sin) and (-sin, cos), and the same negated behind it, so that dataBit * codeCA is an address bit and
 *       u * conj(r) is two packed dot products (v_dot2c_i32_i16), no negation issued per sample.  The chips are the PRN's 32
 *       words.  An SC8 or SC1 view is the same arithmetic on smaller numbers: VIEW only selects the quantiser.
 *   sums: int32 per lane and channel over its 16 samples (a term is below 2^25.1, sixteen of them fit), widened to int64,
 *       summed over the wavefront (butterfly), kept by lane i for channel i while consecutive tiles of a chunk share a
 *       segment, then one 64-bit integer atomic per (channel, segment, chunk) and component.  Integer sums are order-free:
 *       the result does not depend on which wavefront took which chunk.
 */
#ifndef GPSBB_DESPREAD_HIP_H
#define GPSBB_DESPREAD_HIP_H

#include "gpsbb_dense.hip.h"
#include "gpsbb_noise.hip.h"
#include "gpsbb_interf.hip.h"

namespace gpsbb_impl {

constexpr int DS_WG = 256;                /* four wavefronts: the LDS image is small, several workgroups share a CU */
constexpr int DS_WAVES = DS_WG / 64;
constexpr int DS_CHUNK = 4;               /* consecutive tiles a wavefront takes at a time */
constexpr int DS_SC16 = 0;                /* VIEW: DS_SC16, PACK_SC8, PACK_SC1 */

struct DsArgs {
    const uint32_t *iq;          /* the blocks' samples as rendered (Q << 16 | I), block b at b * nsamp; only read */
    unsigned long long *out;     /* [nblocks][nch][nseg][2] (P.i, P.q) as two's complement, zeroed before the launch */
    unsigned long long *n_exact; /* samples that took the exact path (the tests' view of the fallback) */
    int32_t *ctr;                /* [nblocks] next tile to hand out, zeroed before the launch */
    int seg_tiles, nseg, chunk, wgs_per_block;
    int shift8;                  /* PACK_SC8's shift */
    uint32_t danger;             /* a model's low word below this: the sample is recomputed exactly (2 * PD_BAND) */
    NoiseArgs nz;                /* NOISE: sample0 is the position of sample 0 of block 0 */
    const int2 *ntab;
    InterfArgs it;               /* INTERF: the emitters, sample0 and shift as nz's (gpsbb_batch_despread_impaired) */
};

typedef short ds_s16x2 __attribute__((ext_vector_type(2)));

struct DsLds {
    uint2 rep[2][512];                 /* [0][k]: x = (cos, sin) of table index k as an int16 pair, y = (-sin, cos); [1]: negated */
    uint32_t chips[GPSBB_MAX_CHAN][32]; /* bit c & 31 of word c >> 5 = chip c of the channel's PRN (1: codeCA +1) */
};

__device__ __forceinline__ uint32_t ds_pair(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }

/* index (bits 0-8) and sign (bit 9: the replica is negative) of sample n after the state (xt, yt) as the reference has them
 * (c:2697-2737): the exact jump-ahead, for the samples the model cannot vouch for.  nav: bit 0 the data bit in force at the
 * state's sample is -1, bit 1 the one after the next roll-over (at most one between a state and the end of its tiles). */
__device__ __forceinline__ uint32_t ds_exact_sample_body(double xt, double yt, double S, double sc, uint32_t down, uint32_t nav, int n,
                                                         int ny, const uint32_t *chips)
{
    int64_t wraps = 0;
    const double x = code_jump(xt, sc, (int64_t)n, &wraps);
    const uint32_t neg = wraps > 0 ? (nav >> 1) & 1u : nav & 1u;
    const double cp = carr_jump(yt * (1.0 / 512.0), (down ? -S : S) * (1.0 / 512.0), (int64_t)ny);
    const int it = (int)(cp * 512.0) & 511; /* c:2697; carr_phase == 1.0: index 512 defined as 0 */
    const int ci = (int)x;                  /* c:2737 */
    const uint32_t bit = (chips[(ci >> 5) & 31] >> (ci & 31)) & 1u;
    return (uint32_t)it | (((bit ^ 1u) ^ neg) << 9);
}
__device__ __noinline__ uint32_t ds_exact_sample(double xt, double yt, double S, double sc, uint32_t down, uint32_t nav, int n,
                                                 const uint32_t *chips)
{
    return ds_exact_sample_body(xt, yt, S, sc, down, nav, n, n, chips);
}
/* ... behind a carrier granule that is not the code's (ev_carr_log2): the carrier state yt lies ny samples back, the code's n */
__device__ __noinline__ uint32_t ds_exact_sample_2g(double xt, double yt, double S, double sc, uint32_t down, uint32_t nav, int n, int ny,
                                                    const uint32_t *chips)
{
    return ds_exact_sample_body(xt, yt, S, sc, down, nav, n, ny, chips);
}

/* the model's index | sign << 9 of one sample, and whether it can be trusted */
__device__ __forceinline__ uint32_t ds_model_sample(double nn, double nny, double S, double sc, double yg, double xg, uint32_t flip, uint32_t nav,
                                                    const uint32_t *chips, uint32_t danger, bool &bad)
{
    const double y = __fma_rn(nny, S, yg), x = __fma_rn(nn, sc, xg);
    bad = min((uint32_t)__double2loint(y), (uint32_t)__double2loint(x)) < danger;
    const uint32_t it = ((uint32_t)__double2hiint(y) & 511u) ^ flip;
    uint32_t c = (uint32_t)__double2hiint(x) & 0xfffffu;
    const bool rolled = c >= (uint32_t)GPSBB_CA_LEN;
    c -= rolled ? (uint32_t)GPSBB_CA_LEN : 0u;
    const uint32_t bit = (chips[(c >> 5) & 31u] >> (c & 31u)) & 1u;
    const uint32_t neg = rolled ? (nav >> 1) & 1u : nav & 1u;
    return it | (((bit ^ 1u) ^ neg) << 9);
}

/* the carrier tables as the replica image holds them: rep[0][k].x = (cos, sin) of index k as an int16 pair */
struct DsRepTab {
    const uint2 *rep;
    __device__ __forceinline__ void operator()(uint32_t idx, int *c, int *s) const
    {
        const uint32_t v = rep[idx].x;
        *c = (int)(v << 16) >> 16;
        *s = (int)v >> 16;
    }
};

/* what a receiver of the view sees of the rendered pair v at sample n of block b: interference and noise (steps 1-4 of
 * gpsbb_noise_t, with gpsbb_interf_t's J), then the format's quantiser, unpacked, as an int16 pair */
template <int VIEW, bool NOISE, bool INTERF = false>
__device__ __forceinline__ uint32_t ds_view(uint32_t v, unsigned long long pos, const DsArgs &a, const int2 *ntab, const uint2 *rep = nullptr)
{
    int vi = (int)(v << 16) >> 16, vq = (int)v >> 16;
    if (INTERF) {
        int j[2];
        interf_run<1>(a.it, pos, DsRepTab{rep}, j);
        vi += j[0];
        vq += j[1];
        if (!NOISE) {
            uint32_t clip = 0;
            vi = noise_apply(vi, 0, a.it.shift, clip);
            vq = noise_apply(vq, 0, a.it.shift, clip);
        }
    }
    if (NOISE) {
        const unsigned long long s = a.nz.sample0 + pos;
        uint32_t x[4];
        noise_philox((uint32_t)(s >> 1), (uint32_t)(s >> 33), a.nz.key0, a.nz.key1, x);
        const bool odd = (s & 1ull) != 0ull;
        uint32_t clip = 0; /* thrown away: GPSBB_INFO_NOISE_CLIPPED counts what leaves the GPU, not what is looked at */
        vi = noise_apply(vi, noise_n(odd ? x[2] : x[0], ntab, a.nz.s256), a.nz.shift, clip);
        vq = noise_apply(vq, noise_n(odd ? x[3] : x[1], ntab, a.nz.s256), a.nz.shift, clip);
    }
    if (VIEW == PACK_SC8) {
        vi = min(max(vi >> a.shift8, -128), 127);
        vq = min(max(vq >> a.shift8, -128), 127);
    } else if (VIEW == PACK_SC1) {
        vi = vi > 0 ? 1 : -1;
        vq = vq > 0 ? 1 : -1;
    }
    return ds_pair(vi, vq);
}

/* ---- what k_despread (below) and k_despread_lags (gpsbb_despread_lags.hip.h) do alike around their own sums.  Which state serves
 * a tile, and where its row lies, is ev_state_at's and ev_tile_x_row's to say (gpsbb_events.hip.h). ---- */
/* stage, by the whole workgroup of the block with descriptors cb: the carrier table as replica pairs, the block's chips, the noise's knots */
template <bool NOISE>
__device__ __forceinline__ void ds_stage(const BatchDev &p, const DsArgs &a, const gpsbb_chan_t *__restrict__ cb, int tid, DsLds &L, int2 *ntab)
{
    for (int k = tid; k < 512; k += DS_WG) {
        const int c = p.tabs[k], s = p.tabs[512 + k];
        L.rep[0][k] = make_uint2(ds_pair(c, s), ds_pair(-s, c));
        L.rep[1][k] = make_uint2(ds_pair(-c, -s), ds_pair(s, -c));
    }
    for (int k = tid; k < p.nch * 32; k += DS_WG) {
        const int prn = cb[k >> 5].prn;
        L.chips[k >> 5][k & 31] = p.ca_bits[(prn > 0 ? prn : 0) * 32 + (k & 31)];
    }
    if (NOISE)
        for (int k = tid; k < NOISE_KNOTS - 1; k += DS_WG)
            ntab[k] = a.ntab[k];
}
/* bit i: channel i of the block has a PRN */
__device__ __forceinline__ uint32_t ds_active(const gpsbb_chan_t *__restrict__ cb, int nch, int lane)
{
    return (uint32_t)__ballot(lane < nch && cb[lane < nch ? lane : 0].prn > 0);
}
/* the wavefront's next chunk of tiles from block b's counter */
__device__ __forceinline__ int ds_claim(const DsArgs &a, int b, int lane)
{
    int base = 0;
    if (lane == 0)
        base = atomicAdd(&a.ctr[b], a.chunk);
    return __builtin_amdgcn_readfirstlane(base);
}
/* the exact replica (out of line) of the sample n after the code's state and ny after the carrier's: one granule for both, or two */
template <int SG>
__device__ __forceinline__ uint32_t ds_exact(double xt, double yt, double S, double sc, uint32_t down, uint32_t nav, int n, int ny, const uint32_t *chips)
{
    return ev_kind_log2(SG, NCO_CARR) == SG ? ds_exact_sample(xt, yt, S, sc, down, nav, n, chips) : ds_exact_sample_2g(xt, yt, S, sc, down, nav, n, ny, chips);
}
/* the samples this wavefront sent down the exact path, added to the call's count (the tests' view of the fallback) */
__device__ __forceinline__ void ds_count_exact(const DsArgs &a, int lane, unsigned long long n_exact)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        n_exact += (unsigned long long)__shfl_xor((long long)n_exact, off);
    if (lane == 0 && n_exact)
        atomicAdd(a.n_exact, n_exact);
}

/* SG: the batch's state granule (BatchDev::st_log2) */
template <int VIEW, bool NOISE, int SG, bool INTERF = false>
__global__ __launch_bounds__(DS_WG) void k_despread(BatchDev p, DsArgs a)
{
    __shared__ DsLds L;
    __shared__ int2 ntab[NOISE ? NOISE_KNOTS - 1 : 1];
    const int tid = (int)threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.wgs_per_block);
    if (b >= p.nblocks)
        return;
    const gpsbb_chan_t *__restrict__ cb = p.ch + (size_t)b * p.nch;
    const EvConst *__restrict__ kb = p.evc + (size_t)b * p.nch;
    ds_stage<NOISE>(p, a, cb, tid, L, ntab);
    __syncthreads();

    /* ---- from here on every wavefront works alone ---- */
    const int lane = tid & 63;
    const uint32_t act_mask = ds_active(cb, p.nch, lane);
    const int ntw = p.ntiles, nst = SG ? p.nstates : ntw;
    const double *__restrict__ txb = p.tile_x + ev_tile_x_row((size_t)b, p.nch, 0, NCO_CODE, nst);
    const uint32_t *__restrict__ tnb = p.tile_nav + ev_tile_nav_row((size_t)b, p.nch, 0, nst);
    const uint32_t *__restrict__ iqb = a.iq + (size_t)b * p.nsamp;
    const double guard = 0x1p+20 + (double)PD_BAND * 0x1p-32;
    long long run_i = 0, run_q = 0; /* lane i: channel i's sums over the tiles of segment run_seg this wavefront has taken */
    int run_seg = -1;
    unsigned long long n_exact = 0ull;
    auto flush = [&]() {
        if (run_seg >= 0 && lane < p.nch) {
            unsigned long long *o = a.out + (((size_t)b * p.nch + lane) * (size_t)a.nseg + (size_t)run_seg) * 2;
            if (run_i)
                atomicAdd(o, (unsigned long long)run_i);
            if (run_q)
                atomicAdd(o + 1, (unsigned long long)run_q);
        }
        run_i = run_q = 0;
    };
    for (;;) {
        const int base = ds_claim(a, b, lane);
        if (base >= ntw)
            break;
        const int stop = base + a.chunk < ntw ? base + a.chunk : ntw;
        for (int wt = base; wt < stop; wt++) {
            const int seg = wt / a.seg_tiles;
            if (seg != run_seg) {
                flush();
                run_seg = seg;
            }
            /* ---- the lane's 16 samples of the tile, as the receiver sees them: sample wt*TILE + j*64 + lane ---- */
            const int left = p.nsamp - wt * TILE - lane; /* samples j*64 < left exist */
            uint32_t u[SPT];
#pragma unroll
            for (int j = 0; j < SPT; j++)
                u[j] = j * 64 < left ? iqb[(size_t)wt * TILE + j * 64 + lane] : 0u;
#pragma unroll
            for (int j = 0; j < SPT; j++)
                u[j] = j * 64 < left ? ds_view<VIEW, NOISE, INTERF>(u[j], (unsigned long long)b * (unsigned long long)p.nsamp +
                                                                              (unsigned long long)(wt * TILE + j * 64 + lane), a, ntab, L.rep[0])
                                     : 0u; /* a sample that does not exist adds nothing */
            const EvStateAt cx = ev_state_at(SG, NCO_CODE, wt), cy = ev_state_at(SG, NCO_CARR, wt); /* SG is the code's granule */
            const int g = cx.entry, gy = cy.entry, ns = cx.since * TILE + lane, nsy = cy.since * TILE + lane;
            const double n0 = (double)ns, n0y = (double)nsy; /* samples since the state's */
            for (uint32_t mk = act_mask; mk; mk &= mk - 1) {
                const int i = __builtin_ctz(mk);
                const double S = scalar_load(&kb[i].S), sc = scalar_load(&kb[i].sc);
                const uint32_t down = scalar_load(&kb[i].down) != 0 ? 1u : 0u;
                const double xt_s = txb[ev_tile_x_row(0, p.nch, i, NCO_CODE, nst) + g], yt = txb[ev_tile_x_row(0, p.nch, i, NCO_CARR, nst) + gy];
                /* (a granule table's code states carry the data bits in their signs: ev_nav_in_sign) */
                const double xt = ev_nav_in_sign(SG) ? __builtin_fabs(xt_s) : xt_s;
                const uint32_t nav = ev_nav_in_sign(SG) ? ev_nav_of_signs(p, (size_t)b, i, g) : tnb[ev_tile_nav_row(0, p.nch, i, nst) + g];
                const double yg = (down ? 512.0 - yt : yt) + guard, xg = xt + guard;
                const uint32_t flip = down ? 511u : 0u;
                const uint32_t *chips = L.chips[i];
                int pi = 0, pq = 0;
                uint32_t bad = 0u;
#pragma unroll
                for (int j = 0; j < SPT; j++) {
                    bool bj;
                    const uint32_t r = ds_model_sample(n0 + (double)(j * 64), n0y + (double)(j * 64), S, sc, yg, xg, flip, nav, chips, a.danger, bj);
                    bad |= bj ? 1u << j : 0u;
                    const uint2 t = (&L.rep[0][0])[r];
                    pi = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, u[j]), __builtin_bit_cast(ds_s16x2, t.x), pi, false);
                    pq = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, u[j]), __builtin_bit_cast(ds_s16x2, t.y), pq, false);
                }
                /* ---- rare: the samples whose model came within its error of an integer take the exact replica instead ---- */
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad != 0u) != 0ull, 0)) {
#pragma unroll 1
                    for (int j = 0; j < SPT; j++) { /* (one call site, the sample picked by selects: u[] stays in registers) */
                        if (!((bad >> j) & 1u) || j * 64 >= left)
                            continue;
                        uint32_t uw = 0u;
#pragma unroll
                        for (int q = 0; q < SPT; q++)
                            uw = q == j ? u[q] : uw;
                        bool bj;
                        const uint32_t rm = ds_model_sample(n0 + (double)(j * 64), n0y + (double)(j * 64), S, sc, yg, xg, flip, nav, chips, a.danger, bj);
                        const uint32_t re = ds_exact<SG>(xt, yt, S, sc, down, nav, ns + j * 64, nsy + j * 64, chips);
                        const uint2 tm = (&L.rep[0][0])[rm], te = (&L.rep[0][0])[re];
                        const ds_s16x2 uj = __builtin_bit_cast(ds_s16x2, uw);
                        pi += __builtin_amdgcn_sdot2(uj, __builtin_bit_cast(ds_s16x2, te.x), 0, false) -
                              __builtin_amdgcn_sdot2(uj, __builtin_bit_cast(ds_s16x2, tm.x), 0, false);
                        pq += __builtin_amdgcn_sdot2(uj, __builtin_bit_cast(ds_s16x2, te.y), 0, false) -
                              __builtin_amdgcn_sdot2(uj, __builtin_bit_cast(ds_s16x2, tm.y), 0, false);
                        n_exact++;
                    }
                }
                /* ---- widen, sum over the wavefront, lane i keeps channel i ---- */
                long long si = pi, sq = pq;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    si += __shfl_xor(si, off);
                    sq += __shfl_xor(sq, off);
                }
                if (lane == i) {
                    run_i += si;
                    run_q += sq;
                }
            }
        }
    }
    flush();
    ds_count_exact(a, lane, n_exact);
}

} /* namespace gpsbb_impl */
#endif
