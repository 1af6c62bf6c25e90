/*
 * gpsfe.h — host front end for libgpsbb: from {RINEX-2 navigation file, receiver position or motion,
 * start time} to the per-block channel descriptors (gpsbb_chan_t) the IQ fill consumes.
 *
 * This is the part of the reference that stays on the host.  It reproduces,
 * bit for bit, what the reference's main() leaves in chan[] / gain[] before every run of the sample loop:
 *   ephemeris reader           readRinex2 / readRinex3   plutogpssim.c:874-1233, 1241-1610
 *   scenario start / eph set   main()                plutogpssim.c:2497-2597
 *   orbit + clock              satpos                plutogpssim.c:443-546
 *   range, az/el, Klobuchar    computeRange          plutogpssim.c:1691-1747, 1612-1683
 *   nav message                eph2sbf, generateNavMsg, computeChecksum   c:552-723, 1820-1894, 751-814
 *   channel allocation         allocateChannel       plutogpssim.c:1918-1989
 *   per-block seeding          computeCodePhase + gain   plutogpssim.c:1754-1787, 2656-2687
 *   30 s maintenance           main()                plutogpssim.c:2764-2805
 * Plain C, scalar doubles, built -ffp-contract=off -fno-builtin so every libm call and rounding is the
 * reference's.  Checked field by field (bitwise) against descriptor dumps of the reference's own code.
 */
#ifndef GPSFE_H
#define GPSFE_H

#include "gpsbb.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Input that is not valid.  On a valid file the front end is the reference, bit for bit; it departs from the reference on
 * invalid input only, where the reference indexes out of bounds (date2gps with a month of 0, as a trailing blank line
 * gives), never returns (satpos with an eccentricity of 1 or more) or hands out descriptors that are not finite.
 *
 * GPSFE_E_NAVFILE.  An ephemeris record is taken only if it is complete and valid:
 *   - all eight lines are there, none longer than the reader's line buffer (99 characters), and every numeric field of
 *     them is finite (a blank or cut-off field reads 0, as in the reference);
 *   - month 1..12, day 1..31, hour 0..23, minute 0..59, seconds in [0, 61), year 1980 or later, PRN 1..32;
 *   - every value is one its field of the navigation message can hold (IS-GPS-200: the field's bits times its scale factor):
 *     0 <= ecc < 0.5 (32 bits of 2^-33), 0 < sqrt(A) < 8192 (32 bits of 2^-19), 0 <= toe < 604800, |af0| <= 2^-10,
 *     |af1| <= 2^-28, |af2| <= 2^-48, |tgd| <= 2^-24, |crs|, |crc| <= 1024, |cuc|, |cus|, |cic|, |cis| <= 2^-14,
 *     |delta n| <= 2^-28 pi, |omega dot| <= 2^-20 pi, |idot| <= 2^-30 pi, the four angles within one turn (2 pi),
 *     IODE 0..255, IODC 0..1023, codes on L2 0..3, health 0..63, week 0..65535.
 * Reading stops at the first record that fails; that record is not used, the sets read so far are.  A file with more
 * sets than the table holds (13) gives its first 13.  A file that cannot be opened, that is of the other RINEX version, or
 * that yields no valid record is GPSFE_E_NAVFILE.
 * Header: ionosphere or UTC terms that are not finite, or that page 18 cannot hold (alpha 8 bits of 2^-30, 2^-27, 2^-24,
 * 2^-24; beta 8 bits of 2^11, 2^14, 2^16, 2^16; A0 32 bits of 2^-30; A1 24 bits of 2^-50), leave the ionosphere model at
 * its default, as a header without these lines does.
 *
 * GPSFE_E_MOTION.  The motion file ends at the first line that is not four numbers, finite and at most 1e9 m in size, or
 * that is longer than the reader's line buffer; the points read so far are used.  A file that cannot be opened or that yields
 * no point is GPSFE_E_MOTION.
 *
 * The Newton iteration of the orbit is bounded (a valid record never reaches the bound), and the antenna-pattern index is
 * kept within its table.  tests/test_frontend_malformed.py, tests/rinex_mutants.py, tools/fe_asan.c.
 */
#define GPSFE_OK 0
#define GPSFE_E_BADARG (-1)
#define GPSFE_E_NAVFILE (-2)   /* cannot open / not a RINEX GPS nav file of the version asked for / no valid record */
#define GPSFE_E_MOTION (-3)    /* cannot open / no valid point in the user-motion file                */
#define GPSFE_E_TIME (-4)      /* start time outside the ephemeris window (c:2555-2564)             */
#define GPSFE_E_NOEPH (-5)     /* no ephemeris set within an hour of the start time (c:2593-2596)   */
#define GPSFE_E_NOMEM (-6)

typedef struct gpsfe gpsfe_t;

typedef struct gpsfe_config {
    const char *navfile;     /* -e : RINEX navigation file (plain or gzip)                          */
    int rinex3;              /* -3 : the file is RINEX 3 (readRinex3 c:1241-1610) instead of 2      */
    const char *motion_file; /* -u : "t,x,y,z" ECEF at 10 Hz; NULL = static position               */
    int use_ecef;            /* static position given as ECEF (-c) instead of lat,lon,height (-l)  */
    double pos[3];           /* -l: degrees, degrees, metres   /   -c: metres ECEF                  */
    int have_start;          /* -t given                                                            */
    int y, m, d, hh, mm;     /* -t YYYY/MM/DD,hh:mm:ss                                              */
    double sec;
    int time_overwrite;      /* -T : overwrite TOC/TOE to the scenario start time                   */
    int iono_disable;        /* -i                                                                  */
    int max_chan;            /* channels to allocate: 12 in the reference (h:21), up to 16 here     */
    int fixed_carrier;       /* descriptors for GPSBB_FIXED_CARRIER: carr_phase is the 32-bit accumulator
                                value the `#ifndef FLOAT_CARR_PHASE` code initialises at c:1966-1967 */
} gpsfe_config_t;

int gpsfe_open(const gpsfe_config_t *cfg, gpsfe_t **out);
void gpsfe_close(gpsfe_t *fe);
const char *gpsfe_strerror(int err);

/* number of channels (cfg.max_chan) */
int gpsfe_max_chan(const gpsfe_t *fe);

/*
 * Descriptors of the next 0.1 s block (what c:2656-2687 computes) into ch[max_chan], then advance the
 * scenario by one block including the 30-second maintenance (c:2764-2805).
 * ch[i].carr_phase is the value the front end knows: the initial phase of a channel when it was
 * allocated (c:1956-1964) or whatever was fed back with gpsfe_feed_back().  Callers that render the
 * blocks in time order on one handle use GPSBB_CHAIN_CARRIER and never feed back; callers that shard the
 * stream use gpsbb_chain_carrier_host() on the descriptor sequence.
 */
int gpsfe_next_block(gpsfe_t *fe, gpsbb_chan_t *ch);

/* Optional: give the front end the carrier phases the fill left behind (end_state of the block just
 * rendered), exactly as the reference's loop updates chan[i].carr_phase in place. */
int gpsfe_feed_back(gpsfe_t *fe, const gpsbb_chan_state_t *end_state);

/* nblocks consecutive blocks, block-major into ch[nblocks*max_chan] (no feedback).  The blocks between two 30 s
 * maintenances (c:2764-2798) are independent given the ranges at their ends, so they are spread over threads: the same
 * descriptors, bit for bit, as nblocks calls of gpsfe_next_block. */
int gpsfe_generate(gpsfe_t *fe, int nblocks, gpsbb_chan_t *ch);

/*
 * Multipath: up to GPSFE_MAX_ECHOES echoes, each a channel of its own in the reference's arithmetic — the PRN and data
 * words of its satellite, code phase and bit counters of a longer range, a carrier phase of its own, a scaled gain.
 *   slots     echo j owns slot max_chan + j; allocation never sees these slots, so slots 0 .. max_chan-1 hold, bit for bit,
 *             what they hold without echoes.  After the call gpsfe_next_block and gpsfe_generate write gpsfe_block_chans()
 *             descriptors per block and gpsfe_feed_back reads as many end states; gpsfe_max_chan keeps its meaning.
 *   lifetime  live exactly while its PRN holds a direct channel: born in the call that allocates that channel, freed in
 *             the call that frees it; an idle echo's slot has prn = 0, like any free slot.
 *   path      e(k) = extra_m + rate_mps * (k / 10.0) at the start of block k, counted from the scenario's first block.
 *   NCOs      computeCodePhase (c:1754-1787) on the direct channel's two ranges with range + e(k) and range + e(k+1) in
 *             their place: code phase, iword/ibit/icode, f_carr and f_code all come out of that one function; dwrd is
 *             the direct channel's.
 *   carrier   at birth (2 r_ref - (r_xyz + e)) / lambda + phase_cyc, reduced as c:1956-1967 reduces it for both carrier
 *             variants; afterwards the slot chains (or is fed back) like any channel.
 *   gain      the direct channel's (c:2677-2685) * pow(10.0, -atten_db / 20.0).
 * GPSFE_E_BADARG: a prn outside 1..32, extra_m negative, not finite or above 30 000 m (0.1 ms), a rate, attenuation or
 * phase that is not finite, n outside 0..GPSFE_MAX_ECHOES, max_chan + n > GPSBB_MAX_CHAN, a call after the first block.
 * Two echoes of one PRN are allowed; a later call before the first block replaces the earlier one's echoes.
 */
#define GPSFE_MAX_ECHOES 8
typedef struct gpsfe_echo {
    int prn;          /* 1..32: the satellite this echo belongs to                                   */
    double extra_m;   /* extra path at scenario start, metres, >= 0                                  */
    double rate_mps;  /* d(extra path)/dt, m/s: the echo's Doppler offset is -rate_mps / lambda      */
    double atten_db;  /* echo gain = direct gain * 10^(-atten_db / 20)                               */
    double phase_cyc; /* added to the echo's initial carrier phase, cycles (reflection)              */
} gpsfe_echo_t;
int gpsfe_set_echoes(gpsfe_t *fe, const gpsfe_echo_t *e, int n);
int gpsfe_block_chans(const gpsfe_t *fe); /* max_chan + n: descriptors per block from now on */

/* threads gpsfe_generate uses: 0 = the machine's cores up to 16 (default), 1 = none (the reference's one generator thread,
 * c:2286-2289), up to 32 */
int gpsfe_set_threads(gpsfe_t *fe, int nthreads);

/* introspection for tests / logging: current receiver GPS time and the visible-satellite table */
int gpsfe_time(const gpsfe_t *fe, int *week, double *sec);
int gpsfe_channel_info(const gpsfe_t *fe, int i, int *prn, double *az_deg, double *el_deg, double *range_m,
                       double *iono_m);
/* the ephemeris sets the navigation file gave: returns their number and writes the valid satellites of the first `cap`
 * of them to nvalid[] */
int gpsfe_eph_sets(const gpsfe_t *fe, int *nvalid, int cap);

#ifdef __cplusplus
}
#endif
#endif
