/*
 * gpsbb_testhooks.h — exported only so that tests can exercise, on the host and without a GPU, the very
 * same exact-jump-ahead code (gpsbb_nco.h) the device pre-pass runs.  Pure functions: no state, no handle.
 * Not part of the drop-in ABI.
 */
#ifndef GPSBB_TESTHOOKS_H
#define GPSBB_TESTHOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpsbb_test_row {
    int32_t n0;
    uint32_t nav;
    uint64_t xb;
    int64_t inc;
} gpsbb_test_row_t;

/* kind: 0 = code NCO, 1 = carrier NCO */
double gpsbb_test_carr_jump(double x, double s, long long n);
double gpsbb_test_code_jump(double x, double s, long long n, long long *wraps);
int gpsbb_test_build_rows(int kind, double x0, double s, unsigned nav0, int nsamp, gpsbb_test_row_t *rows,
                          int cap, double *x_end, unsigned *nav_end);
/* the builder the device pre-pass uses: xb = bits of x at n0, inc = bits of the double step S; the state at
 * sample n of a row is fma(n - n0, S, x) */
int gpsbb_test_build_rows_f64(int kind, double x0, double s, unsigned nav0, int nsamp, gpsbb_test_row_t *rows,
                              int cap, double *x_end, unsigned *nav_end);
unsigned long long gpsbb_test_row_bound(int kind, double s_abs, int nsamp);
/* the host's drift model of the carrier recurrence: the predicted phase n steps after x0 (not exact: ~1e-14) */
double gpsbb_test_carr_predict(double x0, double s, int n);
/* the fixed-point carrier's table index (fraction included) at the first sample of tile t: what k_tiles / the host hand the
 * model kernels with GPSBB_FIXED_CARRIER */
double gpsbb_test_fixed_tile_index(unsigned ph0, int step, int t);

/* plan_batch (gpsbb.hip) on given descriptors, options and stream carry: what a batch's set-up would decide, without a handle.
 * opt: GPSBB_OPT_SEED_WHERE, _SYNTH_KERNEL, _SKIP_SEED, _CHAIN_WHERE and the batch's table sets at most (a ring slot: 1; else 6).
 * carry: the stream lends its carry (carry_prn, carry_phase in/out as gpsbb_stream_push passes them); fixed_prev_*: the
 * accumulator's chaining state, or NULL.  out: nblocks, nch, nsamp, ntiles, hash(delt), flags, ev, ev_dense, ev_all_dense, laps,
 * host_seed, st_log2, nstates, chain_dev, chain_starts, chain_indep, chain_model, chain_fix_seq, nseg, seg_tiles, fix_wg,
 * fix_chunks, nsets, total_rows, carr_lanes, chain_lanes, cont0_mask, then the 64-bit FNV-1a (0: the plan defines none) of
 * lap_chunk0, h_ch, h_evc, row_off, h_kph0, h_kstep, h_cd, h_start0, h_seed_order, the chain order, carry_phase afterwards.
 * Returns GPSBB_OK or the error batch set-up would return. */
#define GPSBB_TEST_PLAN_NQ 38
struct gpsbb_chan;
int gpsbb_test_plan(const struct gpsbb_chan *ch, int nblocks, int nch, double delt, int nsamp, unsigned flags, const int opt[5],
                    int carry, const int *carry_prn, double *carry_phase, const int *fixed_prev_prn,
                    const uint32_t *fixed_prev_phase, unsigned long long out[GPSBB_TEST_PLAN_NQ]);
/* plan_launch (gpsbb_plan.h) behind plan_batch on the same arguments: what one run of that batch would launch on a device of `cus`
 * CUs (0: unknown), with or without the blocks' digests, skip: as a run GPSBB_OPT_SKIP_SEED leaves without its pre-pass.  out: the
 * GPSBB_TEST_LAUNCH_NF fields of LaunchPlan in its order (prepass kind, lap_wide, lap_merged, lap_fixed, chain, pass_a, pass_b, fix_wg,
 * carr_lanes, walk_lanes, chain_order, seed_ev, seed_lanes, ctr_reset, info_prepass, variant, digest_fused, granule, ev_chunk,
 * pd_danger, helpers, grid_x, grid_y, wg, lds, digest_gx, digest_gy, last_kernel, last_chain_dev), the number of kernels, then per
 * kernel in launch order (at most GPSBB_TEST_LAUNCH_KERNELS) its id (LaunchKernel: family + 256 * instance), grid x, grid y,
 * workgroup, dynamic LDS bytes.  Returns GPSBB_OK or the error batch set-up would return. */
#define GPSBB_TEST_LAUNCH_NF 29
#define GPSBB_TEST_LAUNCH_KERNELS 16
#define GPSBB_TEST_LAUNCH_NQ (GPSBB_TEST_LAUNCH_NF + 1 + 5 * GPSBB_TEST_LAUNCH_KERNELS)
int gpsbb_test_launch_plan(const struct gpsbb_chan *ch, int nblocks, int nch, double delt, int nsamp, unsigned flags, const int opt[5],
                           int carry, const int *carry_prn, double *carry_phase, const int *fixed_prev_prn,
                           const uint32_t *fixed_prev_phase, int cus, int want_digest, int skip, long long out[GPSBB_TEST_LAUNCH_NQ]);
/* plan_push_side (gpsbb_plan.h) on the descriptors of one push of a ring with these flags: on which side gpsbb_stream_push would
 * chain the IEEE carrier.  opt: as above.  out[0]: 0 not at all (no GPSBB_CHAIN_CARRIER, or the accumulator), 1 on host threads,
 * 2 on the device; out[1]: the decision ran plan_begin (its result is handed on to set-up where the side is the device).
 * Returns GPSBB_OK or the error the push would return from there. */
int gpsbb_test_push_side(const struct gpsbb_chan *ch, int nblocks, int nch, double delt, int nsamp, unsigned flags, const int opt[5],
                         int out[2]);
/* plan_chain_only (gpsbb_plan.h) on the arguments of a gpsbb_chain_carrier call and a handle's GPSBB_OPT_SEED_WHERE: what the call
 * would decide before its first HIP call.  out: laps (1 the lap-parallel pre-pass, 0 the row walks), the number of sub-batches,
 * the 64-bit FNV-1a of h_cd and of h_start0, then for each of the first GPSBB_TEST_CHAIN_PLAN_PIECES sub-batches (the count is the
 * true one) b0, nb, cont0_mask and the FNV-1a of its chunk0 (0: the row walks).  Returns GPSBB_OK or the error the call would. */
#define GPSBB_TEST_CHAIN_PLAN_PIECES 64
#define GPSBB_TEST_CHAIN_PLAN_NQ (4 + 4 * GPSBB_TEST_CHAIN_PLAN_PIECES)
int gpsbb_test_chain_plan(const struct gpsbb_chan *ch, int nblocks, int nch, double delt, int nsamp, int seed_where,
                          unsigned long long out[GPSBB_TEST_CHAIN_PLAN_NQ]);

/* The error budgets of the model kernels, measured (gpsbb_modelerr.hip.h): the realised |model - truth| of everything
 * k_synth_ev / k_synth_pd test, over every tile of the batch's last run, per channel index.  Needs a GPU. */
#define GPSBB_TEST_ME_NQ 11  /* maxima per channel: y0, y0/W, tk, tk/W, x0, x0/W, tc, tc/W, pure_y, pure_x, W (units of 2^-32) */
#define GPSBB_TEST_MEC_NQ 4  /* counts per channel: wrong unflagged decisions, lanes flagged, lane-runs looked at, always-exact */
struct gpsbb_batch;
int gpsbb_test_model_err(struct gpsbb_batch *b, double *maxima, unsigned long long *counts, int *which);
/* samples the batch's last gpsbb_batch_despread recomputed with the exact jump-ahead (GPSBB_DS_DANGER raises the threshold) */
unsigned long long gpsbb_test_despread_exact(struct gpsbb_batch *b);
/* ... and what its kernel took, by HIP events on the synthesis stream, in ms (-1: none yet) */
float gpsbb_test_despread_ms(struct gpsbb_batch *b);
/* milliseconds the three kernels of the handle's last gpsbb_device_acquire took (k_acq_chips, k_acq, k_acq_fold), by HIP events */
float gpsbb_test_acquire_ms(struct gpsbb *h);
/* ... and the kernel of its last gpsbb_device_track (k_track) */
float gpsbb_test_track_ms(struct gpsbb *h);
/* ... and of its last gpsbb_device_fir (k_fir); the outputs one of k_fir's workgroups takes (FIR_TILE) */
float gpsbb_test_fir_ms(struct gpsbb *h);
int gpsbb_test_fir_tile(void);
/* ... and of its last gpsbb_device_psd (k_psd, k_psd_fold); the segments of a workgroup's least run at N = 1 << log2n */
float gpsbb_test_psd_ms(struct gpsbb *h);
int gpsbb_test_psd_run(int log2n);
/* ... and of its last gpsbb_device_excise (k_excise, k_exc_fold); the blocks of a workgroup's least run at N = 1 << log2n */
float gpsbb_test_exc_ms(struct gpsbb *h);
int gpsbb_test_exc_run(int log2n);
/* gpsbb_exc.h's plain-C definition (exc_host) over host memory; peak: the largest |component| any inverse step produced */
int gpsbb_test_exc_host(const gpsbb_exc_t *e, const int16_t *w, long nsamp, const int16_t *hist_in, int16_t *out, int16_t *hist_out,
                        uint64_t *clipped, uint64_t *excised, int64_t *peak);
/* ... and of its last gpsbb_device_blank (k_blank, k_exc_fold); the outputs of one of k_blank's tiles, *run (where given): the
 * tiles of a workgroup's least run */
float gpsbb_test_blank_ms(struct gpsbb *h);
int gpsbb_test_blank_tile(int *run);
/* k_blank's output stores from the next call on: non-temporal (1) or plain (0, the product's); process-wide, for tools/blank_rate.py */
void gpsbb_test_blank_nt(int on);
/* gpsbb_blank.h's plain-C definition (blank_host) over host memory */
int gpsbb_test_blank_host(const gpsbb_blank_t *b, const int16_t *w, long nsamp, const int16_t *hist_in, int16_t *out, int16_t *hist_out,
                          uint64_t *blanked, uint64_t *triggers);
/* the state granule of the batch's tile tables as log2 of its tiles: the code rows' (BatchDev::st_log2) and the carrier rows'
 * (ev_carr_log2 of it, gpsbb_events.hip.h) */
int gpsbb_test_state_log2(struct gpsbb_batch *b);
int gpsbb_test_state_log2_carr(struct gpsbb_batch *b);
void gpsbb_test_budgets(double out[3]); /* EV_MODEL_ERR, EV_T_EPS, PD_BAND of this build, in units of 2^-32 */
/* The data bits of a table with a state granule of 2^g tiles, g >= 1, travel in the signs of its code states (ev_nav_in_sign,
 * gpsbb_events.hip.h).  For a state (its bit pattern, non-negative) under a data bit of -1 (minus) or +1: out[0] the pattern as
 * the table of granule g holds it, out[1] the magnitude and out[2] the bit a reader gets back from that, out[3] whether the bit
 * after a roll-over inside entry e of a row that uses `used` entries comes from the block's end state (1) or from the row (0),
 * out[4] the row's entry it comes from (-1: none), out[5] whether granule g keeps its bits this way at all. */
void gpsbb_test_nav_sign(unsigned long long state_bits, int minus, int g, int e, int used, long long out[6]);
/* What the library holds in this process right now: device buffers, pinned host buffers, HIP events — every one made and freed
 * through its owner (DevBuf, PinnedBuf, Event in gpsbb.hip), counted there.  Exported by the product build as well: a cycle of
 * create ... destroy must leave all three where it found them (tests/test_lifecycle_gpu.py). */
void gpsbb_test_live(long long out[3]);

#ifdef __cplusplus
}
#endif
#endif
