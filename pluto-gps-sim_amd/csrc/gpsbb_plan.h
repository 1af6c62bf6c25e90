/*
 * gpsbb_plan.h — how a batch is planned: everything batch set-up decides from the descriptors, the handle's options and a stream's
 * carry, as one pure host function (plan_batch) and the plain structs it fills; ahead of it for a ring's push, on which side
 * the push chains its carrier (plan_push_side); what gpsbb_chain_carrier decides, the chain alone (plan_chain_only); and what one run
 * of a planned batch launches (plan_launch: which pre-pass in which form, which synthesis kernel over which grid with how much LDS,
 * what the handle reports afterwards).  No HIP call, neither the handle nor the batch: gpsbb.hip stages what the plan says
 * (batch_setup) and launches from it (batch_launch); gpsbb_test_plan, gpsbb_test_push_side, gpsbb_test_chain_plan and
 * gpsbb_test_launch_plan run them without a GPU.
 * Included by gpsbb.hip behind the descriptor checks and kernel plans it calls (chan_ok, ev_plan, lap_eligible, lap_bound, lap_unit,
 * row_bound, CarrDrift, channel_threads) and the constants it reads (NSETS, CHAIN_*, the kernels' workgroup sizes and LDS images); not
 * a translation unit of its own.
 */
#ifndef GPSBB_PLAN_H
#define GPSBB_PLAN_H

/* What batch_setup decides and a launch only reads: plan_batch fills it from the descriptors, the options and the stream's carry,
 * without a HIP call.  Nothing after set-up changes it. */
struct BatchPlan {
    /* geometry */
    int nblocks = 0, nch = 0, nsamp = 0, ntiles = 0;
    double delt = 0.0;
    unsigned flags = 0;
    /* which synthesis kernel: the breakpoint kernel (ev: exact tile-start states instead of rows + tile index), with some channel
     * evaluated per sample (ev_dense: k_synth_ev_dense), or every active one (ev_all_dense: k_synth_pd) */
    bool ev = false, ev_dense = false, ev_all_dense = false;
    /* where the pre-pass runs and where the carrier chain is resolved */
    bool laps = false;           /* the lap-parallel pre-pass (gpsbb_laps.hip.h): one lane per lap of every chain */
    bool host_seed = false;      /* the NCO tables of this batch are built on host threads: decided at set-up, like the
                                    chain (a run never re-reads the handle's options) */
    int st_log2 = 0, nstates = 0; /* the state granule of the tile tables (BatchDev::st_log2, ev_state_log2) */
    bool chain_dev = false;      /* GPSBB_CHAIN_CARRIER resolved on the device (gpsbb_walk.hip.h: k_chain_prefix / k_chain_fix) */
    bool chain_starts = false;   /* ... with the per-sample kernel: the chain kernels only fix the blocks' start phases */
    bool chain_indep = false;    /* the chain machinery runs on a batch whose blocks are independent: only the segments of a block are chained */
    bool chain_model = false;    /* pass B starts from the host's drift model of the carrier (no pass A, no k_chain_prefix) */
    bool chain_fix_seq = false;  /* k_chain_fix (blocks in order) instead of k_chain_fix_par: GPSBB_OPT_CHAIN_WHERE 2 */
    int nseg = 1, seg_tiles = 0; /* the device-side chain cuts every block into nseg segments (BatchDev::nseg) */
    int fix_wg = FIXP_WG_BATCH, fix_chunks = 0; /* k_chain_fix_par: lanes per workgroup, chunks per channel */
    /* sizes and lanes */
    int nsets = 2;               /* table sets in use: run k works on set k % nsets */
    uint64_t total_rows = 0;
    int seed_lanes = 0;          /* lanes of the seed plan (h_seed_order): what k_seed / k_walk are launched over */
    int carr_lanes = 0;          /* lanes of the seed plan that walk carrier chains (they come first) */
    int chain_lanes = 0;         /* chain_starts: lanes of the chain order */
    uint32_t cont0_mask = 0;     /* a stream's push: which channels of its first block go on from the push before */
    uint32_t lap_chunk0[2][GPSBB_MAX_CHAN + 1] = {};
};

/* The host images plan_batch leaves for set-up to upload (and for host seeding to read). */
struct PlanImages {
    std::vector<gpsbb_chan_t> h_ch; /* library-owned copy: the caller's array may go away after the call */
    std::vector<EvConst> h_evc;     /* ev: per-channel constants */
    std::vector<uint64_t> row_off;
    std::vector<uint32_t> h_kph0;   /* fixed-point carrier variant: start phase and step per (block, channel) */
    std::vector<int32_t> h_kstep;
    std::vector<ChainDesc> h_cd;    /* what the chain kernels read of the descriptors (24 B per block-channel) */
    std::vector<double> h_start0;   /* rough start phases: where pass A walks from */
    std::vector<int32_t> h_seed_order;  /* lane -> chain plan of k_seed (see BatchDev) */
    std::vector<int32_t> h_chain_order; /* chain_starts: the carrier chains, as k_walk's passes take them */
};

/* What a ring slot lends its batch for one push (gpsbb_stream_push sets it before set-up and clears it after the launch): the
 * carrier continues from the push before. */
struct StreamLink {
    ChainCarryDev *d_carry = nullptr;
    const int *carry_prn = nullptr;        /* in: prn per channel in the last block pushed before */
    double *carry_phase = nullptr;         /* in/out: the host's rough idea of the phase there / after this push */
    hipEvent_t ev_prefix = nullptr, ev_fix = nullptr; /* the stream's: order k_chain_prefix / k_chain_fix across pushes */
    unsigned stream_turn = 0;              /* the stream's push count */
    const int *fixed_prev_prn = nullptr;   /* stream chaining of the fixed-point carrier (host side) */
    const uint32_t *fixed_prev_phase = nullptr;
};

/* ---- plan_batch and its steps ------------------------------------------------------------------------ */

constexpr size_t HOST_SEED_MAX_CHANNELS = 64; /* blocks x channels up to which the host seeds */
/* gpsbb_chain_carrier cuts its blocks into sub-batches that fit its scratch */
constexpr int CHAIN_ONLY_BLOCKS = 16384;  /* blocks per sub-batch: 168 MB of ChainAux at 16 channels */
constexpr double CHAIN_ONLY_LAPS = 6.0e6; /* laps per sub-batch of the lap-parallel chain (40 bytes of scratch each) */

struct PlanIn {
    const gpsbb_chan_t *ch;
    int nblocks, nch;
    double delt;
    int nsamp;
    unsigned flags;
};

/* The handle's options and the measurement knobs the plan consults (experiments build: from the environment), read once. */
struct PlanOpts {
    int seed_where = 0, synth_kernel = 0, chain_where = 0;
    bool skip_seed = false;
    int max_sets = NSETS;
    bool no_laps = false, device_seed_only = false;
    size_t host_seed_max = HOST_SEED_MAX_CHANNELS;
    long state_log2 = 0, indep_min_tiles = 0, seg_rows = 0, walk_lanes = 0;
    long nsets[2] = {3, 4}; /* table sets without / with the device-side chain */
    int chain_only_blocks = CHAIN_ONLY_BLOCKS; /* plan_chain_only's limits: a knob only makes sub-batches smaller (the scratch is */
    double chain_only_laps = CHAIN_ONLY_LAPS;  /* sized by the constants) */
};

static PlanOpts plan_opts(int seed_where, int synth_kernel, bool skip_seed, int chain_where, int max_sets)
{
    PlanOpts o;
    o.seed_where = seed_where;
    o.synth_kernel = synth_kernel;
    o.skip_seed = skip_seed;
    o.chain_where = chain_where;
    o.max_sets = max_sets;
    o.no_laps = GPSBB_KNOB_SET("GPSBB_NO_LAPS");
    o.device_seed_only = GPSBB_KNOB_SET("GPSBB_DEVICE_SEED_ONLY");
    o.host_seed_max = (size_t)GPSBB_KNOB_LONG("GPSBB_HOST_SEED_MAX", HOST_SEED_MAX_CHANNELS);
    o.state_log2 = GPSBB_KNOB_LONG("GPSBB_EV_STATE_LOG2", GPSBB_EV_STATE_LOG2);
    o.indep_min_tiles = GPSBB_KNOB_LONG("GPSBB_INDEP_MIN_TILES", CHAIN_INDEP_MIN_TILES);
    o.seg_rows = GPSBB_KNOB_LONG("GPSBB_SEG_ROWS", CHAIN_SEG_ROWS);
    o.walk_lanes = GPSBB_KNOB_LONG("GPSBB_WALK_LANES", 64);
    /* table sets = pre-passes in flight + 1: the pre-pass of either kernel takes longer than the synthesis it feeds
     * (M1 geometry, per-sample kernel: two sets 6.6e10, three 7.7e10 samples/s), the chained ones longer still */
    o.nsets[0] = GPSBB_KNOB_LONG("GPSBB_NSETS", 3);
    o.nsets[1] = GPSBB_KNOB_LONG("GPSBB_NSETS", 4);
    o.chain_only_blocks = (int)std::min(std::max(GPSBB_KNOB_LONG("GPSBB_CHAIN_ONLY_BLOCKS", CHAIN_ONLY_BLOCKS), 1L), (long)CHAIN_ONLY_BLOCKS);
    o.chain_only_laps = (double)std::min(std::max(GPSBB_KNOB_LONG("GPSBB_CHAIN_ONLY_LAPS", CHAIN_ONLY_LAPS), 1L), (long)CHAIN_ONLY_LAPS);
    return o;
}

static PlanOpts plan_opts(const gpsbb *h, int max_sets)
{
    return plan_opts(h->opt_seed_where, h->opt_synth_kernel, h->opt_skip_seed, h->opt_chain_where, max_sets);
}

/* Which synthesis kernel: the breakpoint kernel (gpsbb_events.hip.h) where every run of SPT samples holds
 * at most one chip change and at most EV_KC_MAX table-index changes and the I sums stay below 2^15. */
static void plan_kernel(BatchPlan &pl, PlanImages &img, const PlanIn &in, const PlanOpts &o)
{
    const gpsbb_chan_t *ch = in.ch;
    const size_t nbc = (size_t)in.nblocks * in.nch;
    const bool fixed = (in.flags & GPSBB_FIXED_CARRIER) != 0;
    pl.ev = o.synth_kernel != 1 && ev_plan(ch, in.nblocks, in.nch, in.delt, img.h_evc, fixed);
    pl.ev_dense = false;
    pl.ev_all_dense = pl.ev;
    if (pl.ev)
        for (size_t k = 0; k < nbc; k++) {
            pl.ev_dense = pl.ev_dense || img.h_evc[k].kc == EV_KC_DENSE;
            pl.ev_all_dense = pl.ev_all_dense && (ch[k].prn <= 0 || img.h_evc[k].kc == EV_KC_DENSE);
        }
    pl.ev_all_dense = pl.ev_all_dense && pl.ev_dense;
    if (fixed && pl.ev_dense && !pl.ev_all_dense) {
        /* The fixed-point carrier has no mixed kernel: k_synth_ev_dense is the IEEE body (a falling phase mirrored as 512 - y,
         * biased change positions), not the accumulator's (512 - 2^-16 - y, exact).  A batch whose channels straddle the
         * one-chip-change-per-run limit (fs within ~50 Hz of 15.5 * 1.023e6 once the code Doppler is in) goes to the stepped
         * kernel. */
        pl.ev = false;
        pl.ev_dense = pl.ev_all_dense = false;
    }
    PUSH_MARK("ev_plan");
}

/* The first step of a plan: the arguments and descriptors checked, the geometry, the synthesis kernel (and with it the EvConst
 * image).  Every error of a plan is returned here, before anything of pl or img is written. */
static int plan_begin(BatchPlan &pl, PlanImages &img, const PlanIn &in, const PlanOpts &o)
{
    if (!in.ch || in.nblocks < 1 || in.nblocks > 65535 || in.nch < 1 || in.nch > GPSBB_MAX_CHAN || in.nsamp < 1 ||
        !(in.delt > 0.0) || !std::isfinite(in.delt) || (in.flags & ~(GPSBB_CHAIN_CARRIER | GPSBB_FIXED_CARRIER)))
        return GPSBB_E_BADARG;
    const size_t nbc = (size_t)in.nblocks * in.nch;
    for (size_t k = 0; k < nbc; k++)
        if (!chan_ok(in.ch[k], in.delt, (in.flags & GPSBB_FIXED_CARRIER) != 0))
            return GPSBB_E_BADCHAN;
    const int ntiles = (in.nsamp + TILE - 1) / TILE;
    if (2ull * nbc * ((unsigned long long)ntiles + 1) >= (1ull << 32))
        return GPSBB_E_NOMEM; /* the tile index is addressed with 32-bit element offsets (16 GiB of it) */
    pl = BatchPlan();
    pl.nblocks = in.nblocks;
    pl.nch = in.nch;
    pl.nsamp = in.nsamp;
    pl.delt = in.delt;
    pl.flags = in.flags;
    pl.ntiles = ntiles;
    plan_kernel(pl, img, in, o);
    return GPSBB_OK;
}

/* What of the lap-parallel pre-pass's eligibility does not depend on the kernel choice: the options, and no step that is tiny.
 * (plan_push_side asks this first and chooses the kernel only where the answer matters.) */
static bool plan_laps_admit(const PlanIn &in, const PlanOpts &o)
{
    return o.seed_where != 1 && o.seed_where != 2 && o.chain_where != 2 && o.chain_where != 3 && !o.no_laps &&
           lap_eligible(in.ch, (size_t)in.nblocks * in.nch, in.delt, (in.flags & GPSBB_FIXED_CARRIER) != 0);
}

/* where the NCO tables of a run are built: by size (default), or as GPSBB_OPT_SEED_WHERE says (tests run both ways) */
static bool host_seeding_wanted(size_t nbc, const PlanOpts &o)
{
    if (o.seed_where)
        return o.seed_where == 2;
    return !o.device_seed_only && nbc <= o.host_seed_max;
}

/* On which side a ring's push chains its IEEE carrier.  NONE: the ring is not chained, or chains the accumulator.  DEVICE: exactly,
 * in parallel over the blocks, the phase carried from push to push in device memory, for either synthesis kernel — the push is planned
 * with the stream's carry (StreamLink::d_carry), from which plan_placement derives chain_dev and never host_seed.  HOST: on host
 * threads, sequential per channel — the push is planned on descriptors that carry every block's start phase, without
 * GPSBB_CHAIN_CARRIER.  A stream may change sides between pushes: the carry then moves across, which costs a synchronisation. */
enum PushChain { PUSH_CHAIN_NONE, PUSH_CHAIN_HOST, PUSH_CHAIN_DEVICE };
struct PushSide {
    PushChain chain = PUSH_CHAIN_NONE;
    bool begun = false; /* the decision took the plan's first step: plan0 (and the images it was given) hold plan_begin's result */
    BatchPlan plan0;
};

/* The device wherever the pre-pass runs there, the host for pushes small enough to be seeded on the host — but for small pushes the
 * lap-parallel pre-pass will take: it costs less than the host threads.  It only takes blocks the model kernels render (a small push
 * of a 1 MS/s stream, which they decline, stays with the host threads instead of the row walks' milliseconds), so plan_begin runs
 * here, once, where the answer hangs on it — the conditions imply the device side unless the kernels decline, so its result is the
 * one the rest of the plan is made for (side.begun). */
static int plan_push_side(PushSide &side, PlanImages &img, const PlanIn &in, const PlanOpts &o)
{
    side = PushSide();
    if (!(in.flags & GPSBB_CHAIN_CARRIER) || (in.flags & GPSBB_FIXED_CARRIER))
        return GPSBB_OK;
    const size_t nbc = (size_t)in.nblocks * in.nch;
    for (size_t k = 0; k < nbc; k++)
        if (!chan_ok(in.ch[k], in.delt))
            return GPSBB_E_BADCHAN;
    bool small_on_dev = nbc <= o.host_seed_max && o.seed_where == 0 && o.synth_kernel != 1 && o.chain_where == 0 &&
                        plan_laps_admit(in, o);
    if (small_on_dev) {
        const int rc = plan_begin(side.plan0, img, in, o);
        if (rc != GPSBB_OK)
            return rc;
        side.begun = true;
        small_on_dev = side.plan0.ev;
    }
    /* (plan_placement's own question: what it would seed on the host without a carry is chained there) */
    const bool dev = o.chain_where != 1 && (!host_seeding_wanted(nbc, o) || small_on_dev);
    side.chain = dev ? PUSH_CHAIN_DEVICE : PUSH_CHAIN_HOST;
    return GPSBB_OK;
}

/* The state granule of a batch's tile tables (BatchDev::st_log2): one exact state per 2^g tiles where the breakpoint kernel proper
 * (k_synth_ev, k_synth_ev_digest) renders behind the lap-parallel pre-pass; one per tile for every other kernel and pre-pass.  The
 * tile anchors k_synth_ev derives from a granule's state (gpsbb_events.hip.h) assume at most one code roll-over from a granule's
 * first sample to its last: 1023 chips take at least 15 800 samples at the steps that kernel admits (sc < 1 / 15.5), against 4 096
 * — checked here for every channel all the same. */
static int ev_state_log2(const BatchPlan &pl, const PlanImages &img, const PlanOpts &o)
{
    if (!pl.ev || !pl.laps || pl.ev_dense || (pl.flags & GPSBB_FIXED_CARRIER))
        return 0;
    long g = o.state_log2;
    g = g < 0 ? 0 : (g > EV_STATE_LOG2_MAX ? EV_STATE_LOG2_MAX : g);
    while (g > 0 && !ev_granule_fits((int)g)) /* (a variant build's smaller budget: make r3budgets) */
        g--;
    const size_t nbc = (size_t)pl.nblocks * pl.nch;
    for (size_t k = 0; k < nbc && g > 0; k++)
        if (!(img.h_evc[k].sc * (double)((TILE << g) + SPT) < (double)(GPSBB_CA_LEN - 1)))
            return 0;
    return (int)g;
}

/* where the pre-pass runs and where the carrier chain is resolved: decided here, once, for all runs of the batch */
static void plan_placement(BatchPlan &pl, const PlanImages &img, const PlanIn &in, const PlanOpts &o, bool carry)
{
    const bool fixed = (in.flags & GPSBB_FIXED_CARRIER) != 0;
    /* on the device: lap-parallel (gpsbb_laps.hip.h) wherever the model kernels render and no step is tiny; the row walks
     * (k_walk and the chain kernels) for the rest and where GPSBB_OPT_SEED_WHERE / _CHAIN_WHERE ask for them.  The lap-parallel
     * pre-pass takes 0.1 ms whatever the size of the batch — less than host threads need for one block (tools/fill_latency.py:
     * 0.25 against 0.33 ms per gpsbb_fill_block of the reference's geometry) — so where it is eligible the size decides nothing. */
    const bool lap_ok = pl.ev && plan_laps_admit(in, o);
    /* (a stream's push on the device side — the carry: PUSH_CHAIN_DEVICE of plan_push_side — stays on the device whatever the
     * size: the row walks where the laps decline, e.g. a rate only the per-sample kernel renders) */
    pl.host_seed = !lap_ok && !carry && host_seeding_wanted((size_t)in.nblocks * in.nch, o);
    pl.laps = lap_ok;
    pl.st_log2 = ev_state_log2(pl, img, o);
    pl.nstates = (pl.ntiles + (1 << pl.st_log2) - 1) >> pl.st_log2;
    const bool chained = !fixed && (in.flags & GPSBB_CHAIN_CARRIER) && (in.nblocks > 1 || carry);
    pl.chain_dev = chained && o.chain_where != 1 && !pl.host_seed;
    pl.chain_fix_seq = o.chain_where == 2;
    pl.chain_starts = pl.chain_dev && !pl.ev;
    pl.chain_model = false; /* decided by plan_segments, once the number of segments is known */
    pl.chain_indep = false;
}

/* The device-side chain cuts blocks into SEGMENTS that are chained like blocks: a walk takes as long as its chain
 * whatever the batch (0.47 us per row; a 5 kHz carrier has 7 000 rows per 0.1 s of signal, at any sample rate), so
 * segments of about CHAIN_SEG_ROWS rows make the two walks of a pre-pass that many times shorter.  (Tried for batches
 * of independent blocks as well, every block's first segment starting a chain: the five dependent kernels of the
 * chain cost more than the shorter walks save — M1 geometry 1.77e11 -> 1.45e11 samples/s — so those keep k_walk<0>.) */
static void plan_segments(BatchPlan &pl, const PlanIn &in, const PlanOpts &o, bool carry)
{
    const gpsbb_chan_t *ch = in.ch;
    const int nblocks = in.nblocks, nsamp = in.nsamp;
    const double delt = in.delt;
    const size_t nbc = (size_t)nblocks * in.nch;
    const bool fixed = (in.flags & GPSBB_FIXED_CARRIER) != 0;
    const bool chained = !fixed && (in.flags & GPSBB_CHAIN_CARRIER) && (nblocks > 1 || carry);
    pl.nseg = 1;
    /* Batches of INDEPENDENT blocks go through the same machinery where the model of the carrier serves (no pass A): every
     * block's first segment starts a chain from its descriptor's phase, the walks are as many times shorter, and the three
     * kernels that follow cost less than a walk of whole blocks — for long blocks (25 MS/s, 2.5 M samples: 4.08e11 ->
     * 4.26e11 samples/s on a resident batch); for the reference's 300 000-sample blocks the fix-up over four thousand short
     * segments costs more than the walks save (1.72e11 -> 1.61e11): those keep k_walk<0>. */
    const bool indep_ok = !chained && !carry && pl.ev && !fixed && !pl.host_seed && o.chain_where == 0 &&
                          pl.ntiles >= (int)o.indep_min_tiles;
    if (!pl.laps && ((pl.chain_dev && !pl.chain_starts) || indep_ok)) { /* (k_seed, the per-sample kernel's pre-pass, walks whole blocks) */
        double rows_max = 0.0;
        for (size_t k = 0; k < nbc; k++)
            if (ch[k].prn > 0) {
                const double sa = std::fabs(ch[k].f_carr * delt);
                const double r = sa > 0.0 ? ((double)nsamp * sa + 1.0) * (2.0 - std::log2(sa)) : 1.0;
                rows_max = r > rows_max ? r : rows_max;
            }
        int n = (int)(rows_max / (double)o.seg_rows + 0.5);
        const int n_cap = pl.ntiles / CHAIN_SEG_MIN_TILES;
        n = n > CHAIN_SEG_MAX ? CHAIN_SEG_MAX : n;
        n = n > n_cap ? n_cap : n;
        n = n < 1 ? 1 : n;
        if (pl.chain_dev) {
            pl.nseg = n;
        } else if (n > 1 && (long)nblocks * n <= CHAIN_MODEL_MAX_SEGS) {
            pl.chain_dev = true;
            pl.chain_indep = true;
            pl.nseg = n;
        }
    }
    pl.seg_tiles = (pl.ntiles + pl.nseg - 1) / pl.nseg;
    pl.nseg = (pl.ntiles + pl.seg_tiles - 1) / pl.seg_tiles; /* no empty last segment */
    /* Pass B's start phases from the host's drift model of the carrier (CarrDrift) instead of a first walk — where the
     * model's error cannot pile up: it is ~6e-15 cycles per segment (partly systematic), and a start phase further than
     * pass B's margin from the truth costs a walk of the segment (about one segment-channel in 10^5 per 1e-12 of error).  So:
     * batches of up to CHAIN_MODEL_MAX_SEGS segments.  Not the pushes of a stream — the belief can only be re-anchored on
     * end states that are a ring's depth of pushes old (measured: 3.3 segment walks per 400-block push, stream 4.48e11 ->
     * 4.26e11 samples/s), and not chains over tens of thousands of blocks (gpsbb_chain_carrier): those keep pass A. */
    pl.chain_model = !pl.laps && pl.chain_dev && !pl.chain_starts && !carry && o.chain_where != 3 &&
                     (long)nblocks * pl.nseg <= CHAIN_MODEL_MAX_SEGS;
    /* k_chain_fix_par, long chains (thousands of segments per channel): fewer, larger chunks — fewer hand-offs */
    if (pl.chain_dev && !pl.laps) {
        pl.fix_wg = nblocks * pl.nseg >= 2048 ? FIXP_WG_ALONE : FIXP_WG_BATCH;
        pl.fix_chunks = (nblocks * pl.nseg + pl.fix_wg - 1) / pl.fix_wg;
    }
}

/* row pool plan: the code chains (block*nch + channel), then the carrier chains ((block*nseg + segment)*nch + channel) */
static void plan_row_pool(BatchPlan &pl, PlanImages &img, const PlanIn &in)
{
    const gpsbb_chan_t *ch = in.ch;
    const int nblocks = in.nblocks, nch = in.nch, nsamp = in.nsamp;
    const double delt = in.delt;
    const size_t nbc = (size_t)nblocks * nch, nvbc = nbc * (size_t)pl.nseg; /* carrier chains: one per (segment, channel) */
    const bool fixed = (in.flags & GPSBB_FIXED_CARRIER) != 0;
    img.row_off.assign(nbc + nvbc + 1, 0);
    uint64_t off = 0;
    for (size_t k = 0; k < nbc && !pl.laps; k++) { /* (the lap-parallel pre-pass keeps no rows) */
        img.row_off[k] = off;
        if (ch[k].prn > 0) {
            off += row_bound(ch[k].f_code * delt, 1023.0, 9, nsamp) + 1;
            if (pl.ev)
                off += (uint64_t)nsamp / (uint64_t)WALK_ROW_MAX + 1; /* k_walk cuts long rows */
        } else {
            off += 1;
        }
    }
    if (!pl.laps) {
        /* a segment's bound depends on the block-channel's step and the segment's length only: one evaluation per
         * block-channel for the full segments, one for the (shorter) last */
        const int full = pl.seg_tiles * TILE, last = nsamp - (pl.nseg - 1) * full;
        const int ns_full = pl.nseg == 1 ? nsamp : full, ns_last = pl.nseg == 1 ? nsamp : last;
        for (int blk = 0; blk < nblocks; blk++)
            for (int sgi = 0; sgi < pl.nseg; sgi++) {
                uint64_t *ro = &img.row_off[nbc + ((size_t)blk * pl.nseg + sgi) * nch];
                const int ns = sgi == pl.nseg - 1 ? ns_last : ns_full;
                for (int i = 0; i < nch; i++) {
                    const gpsbb_chan_t &c = ch[(size_t)blk * nch + i];
                    ro[i] = 0; /* count first, offsets below */
                    if (c.prn > 0 && !fixed) {
                        if (sgi == 0 || sgi == pl.nseg - 1)
                            ro[i] = row_bound(std::fabs(c.f_carr * delt), 1.0, -1, ns) + 1 + (pl.ev ? (uint64_t)ns / (uint64_t)WALK_ROW_MAX + 1 : 0);
                        else
                            ro[i] = img.row_off[nbc + ((size_t)blk * pl.nseg) * nch + i]; /* as the block's first segment */
                    } else {
                        ro[i] = 1;
                    }
                }
            }
        /* (the first segments' entries are read above while later ones are filled: turn counts into offsets afterwards) */
        for (size_t kv = 0; kv < nvbc; kv++) {
            const uint64_t cnt = img.row_off[nbc + kv];
            img.row_off[nbc + kv] = off;
            off += cnt;
        }
    }
    img.row_off[nbc + nvbc] = off;
    pl.total_rows = off;
}

/* start phase and step of the 32-bit accumulator per (block, channel); the chain across blocks is
 * plain modular arithmetic, resolved here (c:2675, 2748) */
static void plan_fixed_point(PlanImages &img, const PlanIn &in, const StreamLink &lk)
{
    const size_t nbc = (size_t)in.nblocks * in.nch;
    img.h_kph0.assign(nbc, 0u);
    img.h_kstep.assign(nbc, 0);
    for (int i = 0; i < in.nch; i++) {
        int prev_prn = lk.fixed_prev_prn ? lk.fixed_prev_prn[i] : 0;
        uint32_t prev_ph = lk.fixed_prev_phase ? lk.fixed_prev_phase[i] : 0u;
        for (int blk = 0; blk < in.nblocks; blk++) {
            const gpsbb_chan_t &c = in.ch[(size_t)blk * in.nch + i];
            const size_t k = (size_t)blk * in.nch + i;
            if (c.prn <= 0) {
                prev_prn = 0;
                continue;
            }
            const volatile double scaled = 512.0 * 65536.0 * c.f_carr * in.delt;
            img.h_kstep[k] = (int)std::round(scaled);
            const bool cont = (in.flags & GPSBB_CHAIN_CARRIER) && c.prn == prev_prn;
            img.h_kph0[k] = cont ? prev_ph : (uint32_t)c.carr_phase;
            prev_ph = img.h_kph0[k] + (uint32_t)in.nsamp * (uint32_t)img.h_kstep[k];
            prev_prn = c.prn;
        }
    }
}

/* The part of the descriptor contract the carrier chain depends on.  Not chan_ok: the node driver chains descriptors whose code
 * fields it has not filled. */
static bool chain_only_chan_ok(const gpsbb_chan_t &d, double delt)
{
    return d.prn == 0 || (d.prn > 0 && d.prn <= 32 && std::isfinite(d.f_carr) && std::isfinite(d.carr_phase) &&
                          !std::signbit(d.carr_phase) && d.carr_phase <= 1.0 && std::fabs(d.f_carr * delt) <= 0.125);
}

/* The carrier chain is resolved exactly on the device, in parallel over the blocks (k_walk pass A,
 * k_chain_prefix, k_walk pass B, k_chain_fix).  All the host contributes is a rough start phase per block:
 * the descriptor's phase carried forward by nsamp*step in plain double arithmetic (good to ~1e-7 cycles
 * after a few hundred blocks; pass A takes it from there).
 * The channels [i0, i1) of images the caller has sized; cont0: their bits of the plan's cont0_mask.
 * ALONE: plan_chain_only's instance (a thread per channel over tens of thousands of blocks: nothing of the general case may cost
 * it anything) — whole blocks, no model, nothing carried in, and the descriptors checked on the way (a batch's are checked by
 * plan_begin): false at the first one chain_only_chan_ok refuses. */
template <bool ALONE>
static bool plan_chain_desc(const BatchPlan &pl, PlanImages &img, const PlanIn &in, const StreamLink &lk, int i0, int i1, uint32_t &cont0)
{
    const int nblocks = in.nblocks, nch = in.nch, nsamp = in.nsamp, nseg = ALONE ? 1 : pl.nseg, full = pl.seg_tiles * TILE;
    const bool model = !ALONE && pl.chain_model, indep = !ALONE && pl.chain_indep, carry = !ALONE && lk.d_carry;
    const double delt = in.delt;
    ChainDesc *const h_cd = img.h_cd.data(); /* (locals: the stores below may alias anything read through a reference) */
    double *const h_start0 = img.h_start0.data();
    for (int i = i0; i < i1; i++) {
        double x = carry && lk.carry_phase ? lk.carry_phase[i] : 0.0;
        int prev_prn = carry && lk.carry_prn ? lk.carry_prn[i] : 0;
        for (int blk = 0; blk < nblocks; blk++) {
            const gpsbb_chan_t &c = in.ch[(size_t)blk * nch + i];
            if (ALONE && !chain_only_chan_ok(c, delt))
                return false;
            const volatile double sk = c.f_carr * delt;
            const CarrDrift drift(model && c.prn > 0 ? (double)sk : 0.0);
            if (c.prn > 0) {
                if (c.prn != prev_prn || indep)
                    x = c.carr_phase;
                else if (blk == 0)
                    cont0 |= 1u << i;
            }
            for (int sgi = 0; sgi < nseg; sgi++) {
                const size_t kv = ((size_t)blk * nseg + sgi) * nch + i;
                h_cd[kv] = ChainDesc{c.f_carr, c.carr_phase /* read for a segment that starts a chain only */, c.prn, indep && sgi == 0 ? 1 : 0};
                h_start0[kv] = c.prn > 0 ? x : 0.0;
                if (c.prn > 0) {
                    const int left = nsamp - sgi * full, ns = nseg == 1 ? nsamp : (left < full ? left : full);
                    if (model && x < 1.0) {
                        x = drift.advance(x, ns, sk);
                    } else {
                        x = x + (double)ns * sk;
                        x -= std::floor(x);
                    }
                }
            }
            prev_prn = c.prn > 0 ? c.prn : 0;
        }
        if (carry && lk.carry_phase)
            lk.carry_phase[i] = x;
    }
    return true;
}

/* The descriptors as the device gets them, and what the carrier of the batch's first block continues: the lap-parallel pre-pass's
 * room (its chains start from the exact phase on the device), the chain descriptors of the row walks, or — blocks consecutive in
 * time whose chain stays on the host — every block's start phase resolved here. */
static void plan_chain(BatchPlan &pl, PlanImages &img, const PlanIn &in, const StreamLink &lk)
{
    const gpsbb_chan_t *ch = in.ch;
    const size_t nbc = (size_t)in.nblocks * in.nch;
    const bool fixed = (in.flags & GPSBB_FIXED_CARRIER) != 0;
    img.h_ch.assign(ch, ch + nbc);
    pl.cont0_mask = 0;
    if (pl.laps) {
        /* the lap-parallel pre-pass: room for the laps of every channel; a stream's push: which channels of its first block go
         * on from the push before (the exact phase is on the device) */
        lap_bound(ch, in.nblocks, in.nch, in.delt, in.nsamp, fixed, pl.lap_chunk0);
        if (pl.chain_dev && lk.d_carry && lk.carry_prn)
            for (int i = 0; i < in.nch; i++)
                if (ch[i].prn > 0 && ch[i].prn == lk.carry_prn[i])
                    pl.cont0_mask |= 1u << i;
    }
    if (pl.chain_dev && !pl.laps) {
        img.h_cd.resize(nbc * (size_t)pl.nseg);
        img.h_start0.resize(nbc * (size_t)pl.nseg);
        plan_chain_desc<false>(pl, img, in, lk, 0, in.nch, pl.cont0_mask);
    }
    if ((in.flags & GPSBB_CHAIN_CARRIER) && !fixed && in.nblocks > 1 && !pl.chain_dev) {
        /* blocks consecutive in time: resolve the carrier phase at the start of every block here, exactly
         * (same jump-ahead as the device, one host thread per channel), so that the device's chains are all
         * independent.  Walking the blocks in order on the device would serialise the whole pre-pass. */
        std::vector<double> seeds(nbc);
        chain_carrier_host(ch, in.nblocks, in.nch, in.delt, in.nsamp, seeds.data(), 0, nullptr);
        for (size_t k = 0; k < nbc; k++)
            if (img.h_ch[k].prn > 0)
                img.h_ch[k].carr_phase = seeds[k];
    }
}

/* The carrier chains (one per (segment, channel), kv = (block*nseg + segment)*nch + channel; nseg = 1: per block) by direction
 * (rising first: by_sign), then by descending |f_carr| — a wavefront runs as long as its longest chain — in CARR_BUCKETS classes of
 * |f_carr| (a counting sort: the plan of a 400-block push with four segments per block orders 25 600 chains, and a comparison sort
 * of them cost more than everything else in the push). */
static std::vector<int32_t> plan_carr_sorted(const gpsbb_chan_t *hc, int nblocks, int nch, int nseg, bool by_sign)
{
    const size_t nbc = (size_t)nblocks * nch;
    std::vector<int32_t> carr(nbc * (size_t)nseg);
    constexpr int CARR_BUCKETS = 512;
    double fmax = 0.0;
    for (size_t k = 0; k < nbc; k++)
        if (hc[k].prn > 0 && std::fabs(hc[k].f_carr) > fmax)
            fmax = std::fabs(hc[k].f_carr);
    const double scale = fmax > 0.0 ? (CARR_BUCKETS - 1) / fmax : 0.0;
    std::vector<uint16_t> key(nbc);
    std::vector<uint32_t> head(2 * CARR_BUCKETS + 2, 0u);
    for (size_t k = 0; k < nbc; k++) {
        unsigned kk;
        if (hc[k].prn <= 0) {
            kk = 2 * CARR_BUCKETS; /* idle channels last */
        } else {
            const unsigned q = (unsigned)(CARR_BUCKETS - 1) - (unsigned)(std::fabs(hc[k].f_carr) * scale);
            kk = (by_sign && std::signbit(hc[k].f_carr) ? CARR_BUCKETS : 0) + (q < (unsigned)CARR_BUCKETS ? q : CARR_BUCKETS - 1);
        }
        key[k] = (uint16_t)kk;
        head[kk + 1] += (uint32_t)nseg;
    }
    for (size_t j = 1; j < head.size(); j++)
        head[j] += head[j - 1];
    for (size_t vb = 0; vb < (size_t)nblocks * nseg; vb++)
        for (int i = 0; i < nch; i++)
            carr[head[key[(vb / nseg) * nch + i]]++] = (int32_t)(vb * nch + i);
    return carr;
}

/* which chain each lane of k_seed walks (BatchDev::seed_order).  k_seed takes as long as its slowest
 * wavefront: rows of its longest chain x the time of one turn of the loop, which grows with the
 * number of lanes that are out of step.  Measured (400 x 16 chains, |f_carr| uniform up to 5 kHz):
 * 6.3 ms in block order, 6.1 ms with the carrier chains by descending |f_carr|, 5.3 ms with the
 * longest of them in wavefronts of few lanes.  (16 chains per wavefront throughout does not help
 * small batches: 16-block ring slots 6.0e9 vs 6.6e9 samples/s.) */
static void plan_seed_order(BatchPlan &pl, PlanImages &img, const PlanOpts &o)
{
    std::vector<int32_t> &order = img.h_seed_order;
    order.clear();
    pl.seed_lanes = 0;
    if (pl.laps) {
        pl.carr_lanes = 0;
        return;
    }
    const size_t nbc = (size_t)pl.nblocks * pl.nch, nvbc = nbc * (size_t)pl.nseg;
    const gpsbb_chan_t *hc = img.h_ch.data();
    /* k_walk runs the two directions in separate loops: keep them in separate wavefronts */
    std::vector<int32_t> carr = plan_carr_sorted(hc, pl.nblocks, pl.nch, pl.nseg, pl.ev);
    auto waves_of = [](std::vector<int32_t> &out, const int32_t *chains, size_t n, size_t per_wave, int32_t add) {
        for (size_t c = 0; c < n; c += per_wave)
            for (size_t l = 0; l < 64; l++)
                out.push_back(l < per_wave && c + l < n ? chains[c + l] + add : -1);
    };
    std::vector<int32_t> code(nbc);
    for (size_t k = 0; k < nbc; k++)
        code[k] = (int32_t)k;
    if (pl.ev) {
        /* k_walk keeps the lanes of a wavefront in lockstep: a turn of its loop costs the same however many
         * lanes take part, so wavefronts are full, the carrier chains by descending |f_carr| (a wavefront runs
         * as long as its longest chain) and the longest ones first */
        waves_of(order, carr.data(), nvbc, (size_t)o.walk_lanes, (int32_t)nbc);
        pl.carr_lanes = (int)order.size();
        waves_of(order, code.data(), nbc, 64, 0);
    } else {
        waves_of(order, code.data(), nbc, 64, 0);
        /* the longest 8 % in wavefronts of 8, the next 16 % in wavefronts of 16, the next 32 % in wavefronts of 32 */
        const size_t n8 = nbc * 8 / 100 / 8 * 8, n16 = nbc * 16 / 100 / 16 * 16, n32 = nbc * 32 / 100 / 32 * 32;
        waves_of(order, carr.data(), n8, 8, (int32_t)nbc);
        waves_of(order, carr.data() + n8, n16, 16, (int32_t)nbc);
        waves_of(order, carr.data() + n8 + n16, n32, 32, (int32_t)nbc);
        waves_of(order, carr.data() + n8 + n16 + n32, nbc - n8 - n16 - n32, 64, (int32_t)nbc);
    }
    pl.seed_lanes = (int)order.size();
    PUSH_MARK("order");
    if (pl.chain_starts) {
        /* the chain's two walks take the carrier chains alone, in lockstep: by direction, then by |f_carr| (nseg = 1
         * here: chains are blocks) */
        std::stable_sort(carr.begin(), carr.end(), [hc](int32_t x, int32_t y) {
            const bool nx = hc[x].prn > 0 && std::signbit(hc[x].f_carr), ny = hc[y].prn > 0 && std::signbit(hc[y].f_carr);
            return nx != ny && ny;
        });
        img.h_chain_order.clear();
        for (size_t c = 0; c < nbc; c += 64)
            for (size_t l = 0; l < 64; l++)
                img.h_chain_order.push_back(c + l < nbc ? carr[c + l] + (int32_t)nbc : -1);
        pl.chain_lanes = (int)img.h_chain_order.size();
    }
}

/* Everything of a plan behind plan_begin.  lk: the stream's carry, present (lk.d_carry) or not; lk.carry_phase is advanced to the
 * end of this batch. */
static void plan_finish(BatchPlan &pl, PlanImages &img, const PlanIn &in, const PlanOpts &o, const StreamLink &lk)
{
    const bool carry = lk.d_carry != nullptr;
    plan_placement(pl, img, in, o, carry);
    plan_segments(pl, in, o, carry);
    pl.nsets = (int)o.nsets[pl.chain_dev ? 1 : 0];
    pl.nsets = pl.nsets < 2 ? 2 : (pl.nsets > NSETS ? NSETS : pl.nsets);
    pl.nsets = pl.nsets > o.max_sets ? o.max_sets : pl.nsets;
    plan_row_pool(pl, img, in);
    if (in.flags & GPSBB_FIXED_CARRIER)
        plan_fixed_point(img, in, lk);
    plan_chain(pl, img, in, lk);
    plan_seed_order(pl, img, o);
}

static int plan_batch(BatchPlan &pl, PlanImages &img, const PlanIn &in, const PlanOpts &o, const StreamLink &lk)
{
    const int rc = plan_begin(pl, img, in, o);
    if (rc == GPSBB_OK)
        plan_finish(pl, img, in, o, lk);
    return rc;
}

/* ---- plan_chain_only: the carrier chain alone (gpsbb_chain_carrier) ------------------------------------ */

/* One sub-batch of the call: nb blocks from block b0 on. */
struct ChainOnlyPiece {
    int b0 = 0, nb = 0;
    uint32_t cont0_mask = 0; /* which channels of its first block go on from the block before it */
    uint32_t chunk0[2][GPSBB_MAX_CHAN + 1] = {}; /* the lap-parallel pre-pass: room for its laps (lap_bound, carriers only) */
};

struct ChainOnlyPlan {
    bool laps = false; /* every piece by the lap-parallel pre-pass; else by the row walks */
    std::vector<ChainOnlyPiece> pieces;
};

/* How many of the blocks from b0 on make the next lap-parallel piece: as many as fit the scratch, by the laps they hold (at least
 * one).  Lanes by the laps per lane a piece of nb + 1 blocks would get: lap_unit grows with the batch, so a block counted with the
 * smaller unit of a smaller batch is over-counted, never under, and the scratch stays within max_laps. */
static int chain_only_lap_blocks(const ChainDesc *cd, int b0, const PlanIn &in, const PlanOpts &o)
{
    double laps = 0.0;
    int nb = 0;
    while (b0 + nb < in.nblocks && nb < o.chain_only_blocks) {
        double l = 0.0;
        const double unit = (double)lap_unit(NCO_CARR, (size_t)(nb + 1) * in.nch);
        for (int i = 0; i < in.nch; i++) {
            const ChainDesc &d = cd[(size_t)(b0 + nb) * in.nch + i];
            if (d.prn > 0)
                l += std::floor((std::floor((double)in.nsamp * std::fabs(d.f_carr * in.delt)) + 1.0) / unit) + 3.0;
        }
        if (nb > 0 && laps + l > o.chain_only_laps)
            break;
        laps += l;
        nb++;
    }
    return nb;
}

/* What gpsbb_chain_carrier decides before its first HIP call: the chain descriptors and rough start phases of all its blocks (img.h_cd,
 * h_start0: nseg = 1, no model, nothing carried in; a thread per channel, the blocks in order), which pre-pass walks them, and the
 * sub-batches that fit the scratch.  Lap-parallel wherever no carrier step is below 2^-50: a fraction of a millisecond per
 * sub-batch whatever its blocks are — the row walks take as long as their longest chain, twice (a feeder that chains every few
 * slots of a stream, the node driver's incremental run, could not live with 8 ms per call).
 * GPSBB_E_BADARG before anything is written; GPSBB_E_BADCHAN leaves cp alone (the images are the threads' scratch by then: the
 * descriptors are checked where they are read, once). */
static int plan_chain_only(ChainOnlyPlan &cp, PlanImages &img, const PlanIn &in, const PlanOpts &o)
{
    if (!in.ch || in.nblocks < 1 || in.nch < 1 || in.nch > GPSBB_MAX_CHAN || in.nsamp < 1 || !(in.delt > 0.0) || !std::isfinite(in.delt))
        return GPSBB_E_BADARG;
    const int nblocks = in.nblocks, nch = in.nch;
    const size_t nbc = (size_t)nblocks * nch;
    img.h_cd.resize(nbc);
    img.h_start0.resize(nbc);
    std::atomic<bool> bad(false);
    channel_threads(nch, nch, [&](int i0, int i1) {
        uint32_t cont0 = 0; /* (nothing is carried in: no channel of block 0 continues) */
        if (!plan_chain_desc<true>(BatchPlan(), img, in, StreamLink(), i0, i1, cont0))
            bad = true;
    });
    if (bad)
        return GPSBB_E_BADCHAN;
    cp.laps = o.seed_where != 1 && !o.no_laps;
    for (size_t k = 0; k < nbc && cp.laps; k++)
        cp.laps = img.h_cd[k].prn <= 0 || lap_carr_step_ok(img.h_cd[k].f_carr, in.delt);
    cp.pieces.clear();
    for (int b0 = 0; b0 < nblocks; b0 += cp.pieces.back().nb) {
        ChainOnlyPiece pc;
        pc.b0 = b0;
        pc.nb = cp.laps ? chain_only_lap_blocks(img.h_cd.data(), b0, in, o) : std::min(nblocks - b0, o.chain_only_blocks);
        for (int i = 0; i < nch && b0 > 0; i++) {
            const int prn = img.h_cd[(size_t)b0 * nch + i].prn;
            if (prn > 0 && prn == img.h_cd[(size_t)(b0 - 1) * nch + i].prn)
                pc.cont0_mask |= 1u << i;
        }
        if (cp.laps)
            lap_bound(in.ch + (size_t)b0 * nch, pc.nb, nch, in.delt, in.nsamp, false, pc.chunk0, true);
        cp.pieces.push_back(pc);
    }
    return GPSBB_OK;
}

/* ---- plan_launch: what one run of a batch launches ------------------------------------------------------ */

/* The CUs a launch is sized for: the device's, or an MI355X's where the handle could not ask. */
static inline long cu_count(int sm_count) { return sm_count > 0 ? sm_count : 256; }

/* What a run knows besides the batch's plan. */
struct LaunchIn {
    long cus = 256;           /* cu_count() */
    bool want_digest = false; /* this run also leaves every block's digest */
    bool carry = false;       /* the batch continues a stream's push (StreamLink::d_carry) */
    bool skip = false;        /* measurement hook (GPSBB_OPT_SKIP_SEED): this run renders from the tables an earlier run left */
};

/* The measurement knobs the launch path consults (experiments build: from the environment), read once. */
struct LaunchOpts {
    int ev_chunk = EV_CHUNK, pd_chunk = PD_CHUNK; /* tiles a wavefront of the model kernels takes at a time */
    bool small_chunks = true;                     /* ... fewer for a batch too small to fill the CUs */
    uint32_t pd_danger = 2u * PD_BAND;            /* (larger: more lanes take the exact path; a test aid) */
    bool lap_wide_set = false, lap_wide = false;  /* k_lap_pass2's wide stores: as asked, else by the sample rate */
    long lap_merge = 0;                           /* 1: both kinds of chain in one grid also for a stream's push; 2: never */
    bool ev_kseed = false;                        /* experiment: the one-kernel pre-pass of the model kernels */
    long ev_helpers = 2, oversub = 12;            /* helper workgroups per CU (model kernels), workgroups per slot (k_synth) */
};

static LaunchOpts launch_opts()
{
    LaunchOpts o;
    o.ev_chunk = (int)GPSBB_KNOB_LONG("GPSBB_EV_CHUNK", EV_CHUNK);
    o.pd_chunk = (int)GPSBB_KNOB_LONG("GPSBB_PD_CHUNK", PD_CHUNK);
    o.small_chunks = GPSBB_KNOB_LONG("GPSBB_SMALL_CHUNKS", 1) != 0;
    o.pd_danger = (uint32_t)GPSBB_KNOB_LONG("GPSBB_PD_DANGER", 2u * PD_BAND);
    o.lap_wide_set = GPSBB_KNOB_SET("GPSBB_LAP_WIDE");
    o.lap_wide = GPSBB_KNOB_LONG("GPSBB_LAP_WIDE", 0) != 0;
    o.lap_merge = GPSBB_KNOB_LONG("GPSBB_LAP_MERGE", 0);
    o.ev_kseed = GPSBB_KNOB_SET("GPSBB_EV_KSEED");
    o.ev_helpers = GPSBB_KNOB_LONG("GPSBB_EV_HELPERS", 2);
    o.oversub = GPSBB_KNOB_LONG("GPSBB_OVERSUB", 12);
    return o;
}

enum PrepassKind {
    PREPASS_SKIP,  /* none: the tables are there */
    PREPASS_HOST,  /* host threads build the tables and upload them */
    PREPASS_LAPS,  /* lap-parallel (gpsbb_laps.hip.h) */
    PREPASS_WALKS, /* the row walks for the model kernels: k_walk<0>, or the chain's walks, then k_tiles */
    PREPASS_SEED   /* k_seed: behind a start-phase chain (the per-sample kernel, chain_starts), or alone */
};

/* Dynamic LDS of a synthesis kernel, by GPSBB_VARIANT_*: one workgroup of the model kernels fits a CU (140 - 156 KB) */
static constexpr int synth_lds(int variant)
{
    return variant == GPSBB_VARIANT_SYNTH      ? (int)sizeof(SynthLds)
           : variant == GPSBB_VARIANT_EV_DENSE ? (int)sizeof(EvLds) + EV_PICK_LDS
           : variant == GPSBB_VARIANT_PD_WIDE  ? (int)sizeof(PdLds<true>) + EV_PICK_LDS
           : variant == GPSBB_VARIANT_PD_NARROW ? (int)sizeof(PdLds<false>) + EV_PICK_LDS
                                                : (int)sizeof(EvLdsLean) + EV_PICK_LDS;
}

/* Everything one run decides: which pre-pass in which form, which synthesis kernel over which grid, what the handle reports
 * afterwards.  plan_launch fills it without a HIP call; prepass_launch and synth_launch only read it. */
struct LaunchPlan {
    PrepassKind prepass = PREPASS_SKIP;
    /* PREPASS_LAPS */
    bool lap_wide = false;   /* pass 2 writes the tile states in 32- / 16-byte pieces (k_lap_pass2<., true>) */
    bool lap_merged = false; /* both kinds of chain in one grid per step: five launches instead of ten */
    bool lap_fixed = false;  /* the accumulator's carrier: no chain to walk, k_lap_plan<NCO_CARR> and k_lap_fixed_tiles */
    /* PREPASS_WALKS, PREPASS_SEED: walk_chain_launch's arguments */
    bool chain = false;       /* the carrier chain's walks run */
    bool pass_a = false;      /* ... with pass A and the prefix (else from the host's drift model) */
    int pass_b = 0;           /* k_walk<2> leaves rows, k_walk<3> the blocks' start phases only */
    int fix_wg = 0;           /* k_chain_fix_par's workgroup; 0: k_chain_fix, the blocks in order */
    int carr_lanes = 0;       /* pass A's lanes */
    int walk_lanes = 0;       /* pass B's lanes */
    bool chain_order = false; /* the walks take the chain order (BatchPlan::chain_lanes), not the seed order */
    bool seed_ev = false;     /* PREPASS_SEED: k_seed<true> */
    int seed_lanes = 0;       /* BatchDev::seed_lanes: lanes of k_seed and k_walk<0> */
    bool ctr_reset = false;   /* the pre-pass zeroes the set's tile counters (k_lap_plan, k_tiles); else a memset does */
    int info_prepass = 1;     /* GPSBB_INFO_PREPASS */
    /* synthesis */
    int variant = 0;           /* GPSBB_VARIANT_*: GPSBB_INFO_LAST_VARIANT */
    bool digest_fused = false; /* the kernel leaves the blocks' digests itself */
    int granule = 0;           /* log2 of the tiles per exact state (BatchPlan::st_log2): k_synth_ev's instance */
    int ev_chunk = 1;
    uint32_t pd_danger = 0;
    long helpers = 0;          /* model kernels: workgroups beyond one per block */
    unsigned grid_x = 0, grid_y = 1;
    int wg = 0, lds = 0;
    unsigned digest_gx = 0, digest_gy = 0; /* k_block_digest behind the kernel; 0: none */
    int last_kernel = 0, last_chain_dev = 0; /* GPSBB_INFO_LAST_KERNEL, _CHAIN_ON_DEVICE */
};

static LaunchPlan plan_launch(const BatchPlan &pl, const LaunchIn &in, const LaunchOpts &o)
{
    LaunchPlan lp;
    const bool fixed = (pl.flags & GPSBB_FIXED_CARRIER) != 0;
    lp.seed_lanes = pl.seed_lanes;
    lp.info_prepass = pl.host_seed ? 2 : (pl.ev && pl.laps ? 3 : 1);
    if (in.skip) {
        lp.prepass = PREPASS_SKIP;
    } else if (pl.host_seed) {
        lp.prepass = PREPASS_HOST;
    } else if (pl.ev && pl.laps) {
        /* A batch that continues nothing (no stream carry: the drop-in call's block, resident batches): both kinds in one grid per
         * step — the chain of small launches IS the latency of a small batch's pre-pass (one block of the reference's geometry:
         * 98 -> 50 us), and a big batch's two plan kernels (16 wavefronts each, 0.1 - 0.2 ms) run side by side.  A stream's pushes
         * keep the kinds apart: their code chains wait for nobody, their carriers for the push before.
         * Wide stores where the geometry has several tiles per lap (a code period is 1023 chips / (1.023e6 * delt) samples); at the
         * reference's 2.6 MS/s a period is 2.5 tiles and the plain loop is the faster one. */
        lp.prepass = PREPASS_LAPS;
        lp.lap_wide = o.lap_wide_set ? o.lap_wide : pl.delt <= 1.0 / 8.0e6;
        lp.lap_merged = !fixed && (!in.carry || o.lap_merge == 1) && o.lap_merge != 2;
        lp.lap_fixed = fixed;
        lp.ctr_reset = true;
    } else if (pl.ev && !o.ev_kseed) {
        lp.prepass = PREPASS_WALKS;
        lp.ctr_reset = true;
        if (pl.chain_dev) { /* (else k_walk<0> over the seed order) */
            lp.chain = true;
            lp.pass_a = !pl.chain_model;
            lp.pass_b = 2;
            lp.carr_lanes = pl.carr_lanes;
            lp.walk_lanes = pl.seed_lanes;
        }
    } else {
        lp.prepass = PREPASS_SEED;
        lp.seed_ev = pl.ev;
        if (!pl.ev && pl.chain_starts) {
            /* the carrier chained on the device for the per-sample kernel: pass A, prefix, pass B without rows and the fix-up put
             * the exact start phase of every block into its descriptor; k_seed then sees independent blocks */
            lp.chain = lp.chain_order = lp.pass_a = true;
            lp.pass_b = 3;
            lp.carr_lanes = lp.walk_lanes = pl.chain_lanes;
        }
    }
    if (lp.chain) /* k_chain_fix_par in workgroups of fix_wg lanes, or (0) k_chain_fix, the blocks in order */
        lp.fix_wg = pl.chain_fix_seq ? 0 : pl.fix_wg;

    lp.last_chain_dev = pl.chain_dev && !pl.chain_indep ? 1 : 0;
    lp.granule = pl.st_log2;
    lp.pd_danger = o.pd_danger;
    /* a batch too small to give every CU a workgroup's worth of chunks (the drop-in call's one block: 293 tiles) hands its tiles out
     * in smaller chunks, down to one at a time: twice the workgroups, half the tiles each (0.116 -> 0.110 ms for the reference's
     * block rendered into a registered buffer) */
    int ev_chunk = pl.ev_all_dense ? o.pd_chunk : o.ev_chunk;
    while (ev_chunk > 1 && o.small_chunks && (long)pl.nblocks * (((long)pl.ntiles + ev_chunk - 1) / ev_chunk) < in.cus * EV_WAVES)
        ev_chunk--;
    lp.ev_chunk = ev_chunk < 1 ? 1 : ev_chunk;
    if (pl.ev) {
        /* Grid = the blocks' primaries, then the helpers (ev_pick_block: a helper joins one of the blocks that still have tiles to
         * hand out, chosen when it starts): as many as can be useful when there are few blocks (never more workgroups per block than
         * there are chunks of tiles per wavefront), else enough to keep every CU busy through the end of the launch — the last round
         * of blocks and then what is left of it take the CUs twice over. */
        lp.variant = pl.ev_all_dense ? (pl.nch <= PD_WIDE_CHAN ? GPSBB_VARIANT_PD_WIDE : GPSBB_VARIANT_PD_NARROW)
                                     : (pl.ev_dense ? GPSBB_VARIANT_EV_DENSE : (fixed ? GPSBB_VARIANT_EV_FIXED : GPSBB_VARIANT_EV));
        lp.last_kernel = 2;
        lp.digest_fused = in.want_digest && (pl.ev_all_dense || lp.variant == GPSBB_VARIANT_EV);
        const long chunks = ((long)pl.ntiles + lp.ev_chunk - 1) / lp.ev_chunk;
        const long max_useful = (chunks + EV_WAVES - 1) / EV_WAVES;
        lp.helpers = std::max(0L, std::min((long)pl.nblocks * (max_useful - 1), in.cus * o.ev_helpers));
        lp.grid_x = (unsigned)(pl.nblocks + lp.helpers);
        lp.wg = EV_WG;
    } else {
        /* Workgroups per block: enough of them to oversubscribe the chip ~3x (tiles are handed out dynamically in chunks, so the
         * tail is short), never more than there are chunks; the per-block LDS tables (amplitude LUT, chips, nav words) are then
         * built few times per block. */
        lp.variant = GPSBB_VARIANT_SYNTH;
        lp.last_kernel = 1;
        const long chunks = ((long)pl.ntiles + TILE_CHUNK - 1) / TILE_CHUNK;
        const long max_useful = (chunks + WAVES_PER_WG - 1) / WAVES_PER_WG;
        const long want = (in.cus * 2 * o.oversub + pl.nblocks - 1) / pl.nblocks;
        lp.grid_x = (unsigned)(int)(want < 1 ? 1 : (want > max_useful ? max_useful : want));
        lp.grid_y = (unsigned)pl.nblocks;
        lp.wg = TILE_THREADS;
    }
    lp.lds = synth_lds(lp.variant);
    if (in.want_digest && !lp.digest_fused) {
        /* a synthesis kernel without a digesting variant: the blocks read back behind it, on its stream */
        const long max_chunks = ((long)pl.nsamp + 1023) / 1024;
        const long chunks = (2048 + pl.nblocks - 1) / pl.nblocks;
        lp.digest_gx = (unsigned)(chunks > max_chunks ? max_chunks : (chunks < 1 ? 1 : chunks));
        lp.digest_gy = (unsigned)pl.nblocks;
    }
    return lp;
}

/* The kernels of a run by name, for whoever asks what a plan launches (gpsbb_test_launch_plan): a family, and from bit 8 up the
 * instance — the lap kernels' kind (NCO_CODE, NCO_CARR, 2: both in one grid; k_lap_pass2 also wide << 2 and the granule << 3), k_walk's
 * pass, k_chain_fix_par's workgroup, k_seed<true> 1, the synthesis kernels' granule and digest << 2. */
enum LaunchKernel {
    LK_LAP_PLAN = 1, LK_LAP_PASS1, LK_LAP_SCAN, LK_LAP_PASS2, LK_LAP_REPAIR, LK_LAP_FIXED_TILES, LK_WALK, LK_CHAIN_PREFIX, LK_CHAIN_FIX,
    LK_CHAIN_FIX_PAR, LK_TILES, LK_SEED, LK_BLOCK_DIGEST,
    LK_SYNTH0 = 100 /* + GPSBB_VARIANT_* */
};
struct LaunchRec {
    int id;
    unsigned gx, gy;
    int wg, lds;
};

/* What prepass_launch and synth_launch (with lap_chain_launch and walk_chain_launch) put on their streams for this plan, in order. */
[[maybe_unused]] static std::vector<LaunchRec> launch_list(const BatchPlan &pl, const LaunchPlan &lp)
{
    std::vector<LaunchRec> v;
    auto add = [&v](int family, int inst, unsigned gx, unsigned gy, int wg, int lds) { v.push_back(LaunchRec{family | inst << 8, gx, gy, wg, lds}); };
    const unsigned nch = (unsigned)pl.nch, nbc = (unsigned)pl.nblocks * nch;
    auto laps = [&](int kind) {
        unsigned chunks = 0;
        for (int k = 0; k < 2; k++)
            if (kind == k || kind == 2)
                chunks += pl.lap_chunk0[k][nch] - pl.lap_chunk0[k][0];
        const unsigned per_chan = kind == 2 ? 2 * nch : nch;
        add(LK_LAP_PLAN, kind, per_chan, 1, 64, 0);
        add(LK_LAP_PASS1, kind, chunks, 1, LAP_WG, 0);
        add(LK_LAP_SCAN, kind, per_chan, 1, 64, 0);
        add(LK_LAP_PASS2, kind | (lp.lap_wide ? 4 : 0) | lp.granule << 3, chunks, 1, LAP_WG, 0);
        add(LK_LAP_REPAIR, kind, per_chan, 1, 64, 0);
    };
    if (lp.chain) {
        if (lp.pass_a) {
            add(LK_WALK, 1, (unsigned)(lp.carr_lanes + GPSBB_WALK_WG - 1) / GPSBB_WALK_WG, 1, GPSBB_WALK_WG, 0);
            add(LK_CHAIN_PREFIX, 0, nch, 1, PREFIX_WG, 0);
        }
        add(LK_WALK, lp.pass_b, (unsigned)(lp.walk_lanes + GPSBB_WALK_WG - 1) / GPSBB_WALK_WG, 1, GPSBB_WALK_WG, 0);
        if (lp.fix_wg == 0)
            add(LK_CHAIN_FIX, 0, 1, 1, 64, 0);
        else
            add(LK_CHAIN_FIX_PAR, lp.fix_wg, nch, (unsigned)pl.fix_chunks, lp.fix_wg, 0);
    }
    switch (lp.prepass) {
    case PREPASS_SKIP:
    case PREPASS_HOST:
        break;
    case PREPASS_LAPS:
        if (!lp.lap_merged)
            laps(NCO_CODE);
        if (lp.lap_fixed) {
            add(LK_LAP_PLAN, NCO_CARR, nch, 1, 64, 0);
            add(LK_LAP_FIXED_TILES, 0, nbc, 1, 256, 0);
        } else {
            laps(lp.lap_merged ? 2 : NCO_CARR);
        }
        break;
    case PREPASS_WALKS:
        if (!lp.chain)
            add(LK_WALK, 0, (unsigned)(lp.seed_lanes + GPSBB_WALK_WG - 1) / GPSBB_WALK_WG, 1, GPSBB_WALK_WG, 0);
        add(LK_TILES, 0, (1 + (unsigned)pl.nseg) * nbc, 1, GPSBB_TILES_WG, 0);
        break;
    case PREPASS_SEED:
        add(LK_SEED, lp.seed_ev ? 1 : 0, (unsigned)(lp.seed_lanes + GPSBB_SEED_WG - 1) / GPSBB_SEED_WG, 1, GPSBB_SEED_WG, 0);
        break;
    }
    add(LK_SYNTH0 + lp.variant, lp.granule | (lp.digest_fused ? 4 : 0), lp.grid_x, lp.grid_y, lp.wg, lp.lds);
    if (lp.digest_gx)
        add(LK_BLOCK_DIGEST, 0, lp.digest_gx, lp.digest_gy, 256, 0);
    return v;
}

#endif
