/*
 * gpsbb-sim — end-to-end generator: RINEX-2 navigation file + position/motion -> int16 I/Q file, with the
 * reference's own program structure (front end -> fill -> TX hand-off) and the fill done on an MI355X.
 *
 *   gpsbb-sim -e nav.14n [-l lat,lon,h | -c x,y,z | -u motion.csv] [-t Y/M/D,h:m:s] [-T] [-i] [-3]
 *             [-s fs_hz] [-d seconds] [-n samples_per_block] [-N channels] [-g gpu] [-F] [-b 1|8|16] [-q shift]
 *             [-D decim[,ntaps[,cutoff[,atten_db]]]] -o out.bin
 *
 * Options mirror the reference's (plutogpssim.c:1991-2012, 2296-2390) where they concern the signal; the
 * Pluto-specific ones (-A -B -U -N host) have no meaning here.  -n defaults to 300000, the reference's
 * fixed block (plutogpssim.c:43-44); "-n 0" means fs/10 (time-continuous blocks, gps-sdr-sim semantics).
 * The main loop below is the reference's (c:2655-2806) with the inline sample loop replaced by
 * gpsbb_fill_block(): same mutex/condvar hand-off, same per-block front-end update, carrier phase fed back.
 * -F ("fast") produces the same bytes faster than real time's structure allows: the front end runs ahead,
 * blocks go through the streaming ring (gpsbb_stream_*, carrier chained exactly on host threads, pinned
 * device-to-host gather on a side stream) and are written as they pop.
 * -G N renders through the node driver (include/gpsbb_node.h): one producer thread + handle + ring per shard on the GPUs
 * "-g a,b,c" names (default 0 .. N-1; an ordinal may repeat), ONE output: a regular file is written with pwrite() as slots
 * complete (GPSBB_NODE_INDEXED), a pipe in stream order.  The stream is fed INCREMENTALLY (gpsbb_node_begin / _feed / _end):
 * the front end makes the descriptors of a few slots, feeds them, and goes round again like the reference's loop — the slots go
 * round the GPUs, each from the exact carrier phase the feeder chained, and the memory used does not grow with -d.
 * -G N -C: N CONTIGUOUS time shards instead (BASELINE configs[4]'s layout; gpsbb_node_run: the whole descriptor sequence up
 * front, each shard seeded by the device-side chain over everything before it); -C -I: the whole sequence up front, slots round
 * the GPUs (GPSBB_NODE_INTERLEAVED).
 * -P usec paces the consumer like the radio does: the TX surface's sink takes one block every `usec` microseconds (the
 * reference's iio_buffer_push blocks until the hardware has room, c:2152; 100000 = real time, less = compressed time), counts
 * the blocks that were not there when their turn came (under-runs) and, with -S file, writes the latency distribution of
 * the drop-in call gpsbb_fill_block (p50 / p99 / max over all blocks) as JSON.  -Q n: blocks the device queues (libiio's
 * kernel buffers: 4 by default; a push only blocks when all are taken).  -R: do not register iq_buff with the library
 * (gpsbb_host_register: by default the drop-in call renders straight into it; with -R it ends with a copy, as for any buffer).  -k a,b,c keeps only those blocks in the
 * output file (a soak of hours of signal need not write them all).
 * -b 8 / -b 1 write gps-sdr-sim's smaller sample formats on every path (include/gpsbb.h GPSBB_OUT_*): 8-bit interleaved I/Q,
 * clamp(v >> shift, -128, 127) with -q shift (default 5: no component of the reference's tables clips at 16 channels; gps-sdr-sim
 * fixes 4 and wraps), or 1-bit packed I/Q (v > 0, MSB first; nsamp % 4 == 0).  The GPU packs them on their way to the host, so
 * fewer bytes cross the bus.  The single-handle paths report how many 8-bit components saturated.  Default -b 16: int16 as ever.
 * -W cn0[,shift] adds receiver noise (include/gpsbb.h gpsbb_noise_t) at a C/N0 of cn0 dB-Hz for a gain-1.0 channel (the reference's
 * zenith normalisation, path loss 1.0 at 20 200 km), w = sat16((v + N) >> shift) with shift 0..7 (default 0) before the sample
 * format packs it; -w seed picks the noise (default 1).  Block b is at stream position b * nsamp on every path, so -k keeps the
 * bytes of the full file.  The single-handle paths report how many components the noise saturated.
 * -J cw,js_db,f_hz[,pulse_period_s,duty] and -J chirp,js_db,f0_hz,f1_hz,sweep_s[,pulse_period_s,duty], up to four times, add
 * interference (include/gpsbb.h gpsbb_interf_t): J/S in dB against a gain-1.0 channel, a tone at f_hz or a sawtooth sweep from
 * f0_hz to f1_hz every sweep_s seconds, optionally pulsed.  It goes in where the noise goes, w = sat16((v + N + J) >> shift); with
 * -W the shift is -W's, without it -j shift (0..7, default 0).  The same bytes on every path, as for -W.
 * -A clip_ppm chooses both shifts from a measurement (include/gpsbb.h gpsbb_level_t) instead of taking them from -W cn0,shift / -j
 * and -q: before generating, the scenario's first min(blocks, 10) blocks are rendered as a resident batch, measured with the
 * run's own -W noise and -J emitters from position 0 (gpsbb_device_level) and the smallest shifts whose predicted clips stay
 * within clip_ppm parts per million are taken (gpsbb_level_choose; 100 is the usual budget).  The run then goes on exactly as if
 * those shifts had been given: the bytes are those of the explicit options, on every path.  The choice is made once, from the
 * first second: a power change later in the run shows up in the clip counters, not in the scale.
 * -D decim[,ntaps[,cutoff[,atten_db]]] puts a front-end filter before the sample format (include/gpsbb.h gpsbb_device_fir): the front
 * end and the render run at -s times decim (-n counts samples of the file: a block is rendered decim times as long), a Kaiser-windowed
 * sinc of ntaps taps (default 8 * decim + 1; gpsbb_fir_make: cutoff as a fraction of the file's Nyquist rate, default 0.8, and 60 dB)
 * band-limits it, every decim-th output is kept, and the file is written at -s in the -b format.  -W and -J apply at the rendered
 * rate, in the filter's view of its input.  A path of its own from public calls: a device-only ring with chained pushes, per popped
 * slot gpsbb_device_fir with the history carried from slot to slot, then gpsbb_device_pack and the write.  Not together with -A
 * (which measures the level before the filter), -P, -k, -S, -R or -G.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "gpsbb.h"
#include "gpsbb_node.h"
#include "gpsbb_tx.h"
#include "gpsfe.h"

/* the node driver's one consumer: a file (random access) or a pipe (ordered) */
struct node_out {
    FILE *f;
    int fd;         /* >= 0: pwrite at the block's offset */
    size_t bytes;   /* per block, in the output format */
};

static int node_sink(void *user, const int16_t *iq, long first_block, int nblocks, int shard)
{
    struct node_out *o = user;
    (void)shard;
    const size_t bytes = (size_t)nblocks * o->bytes;
    if (o->fd >= 0) {
        const char *p = (const char *)iq;
        off_t at = (off_t)first_block * (off_t)o->bytes;
        size_t left = bytes;
        while (left) {
            const ssize_t w = pwrite(o->fd, p, left, at);
            if (w <= 0)
                return -1;
            p += w;
            at += w;
            left -= (size_t)w;
        }
        return 0;
    }
    return fwrite(iq, 1, bytes, o->f) == bytes ? 0 : -1;
}

/* the paced consumer of the soak: what sits behind the TX surface instead of the Pluto */
struct paced_sink {
    FILE *f;
    size_t bytes;           /* of a block, in the output format */
    long period_ns;         /* 0: not paced */
    int queue;              /* blocks the device holds: libiio hands a pushed buffer to the kernel and blocks only when all
                               of its kernel buffers (4 by default) are queued, so the generator may run that far ahead */
    long keep[64];
    int nkeep;              /* 0: keep everything */
    long seen;              /* blocks taken so far */
    long underruns;         /* blocks that arrived after their slot had begun */
    double worst_late_ms;
    struct timespec t0;     /* the first block's arrival: slot k begins at t0 + k * period */
};

static double ts_ms(const struct timespec *a, const struct timespec *b)
{
    return (double)(a->tv_sec - b->tv_sec) * 1e3 + (double)(a->tv_nsec - b->tv_nsec) * 1e-6;
}

static int paced_push(void *user, const int16_t *iq, size_t nsamp)
{
    struct paced_sink *p = user;
    const long k = p->seen++;
    if (p->period_ns > 0) {
        struct timespec now;
        clock_gettime(CLOCK_MONOTONIC, &now);
        if (k == 0)
            p->t0 = now;
        /* block k goes on the air at t0 + k * period; the push returns when the device has room again, i.e. when block
         * k - (queue - 1) has started playing */
        struct timespec due = p->t0, room = p->t0;
        const long long ns = (long long)p->t0.tv_nsec + (long long)k * p->period_ns;
        due.tv_sec += (time_t)(ns / 1000000000LL);
        due.tv_nsec = (long)(ns % 1000000000LL);
        const long long kr = k - (p->queue - 1) > 0 ? k - (p->queue - 1) : 0;
        const long long nr = (long long)p->t0.tv_nsec + kr * p->period_ns;
        room.tv_sec += (time_t)(nr / 1000000000LL);
        room.tv_nsec = (long)(nr % 1000000000LL);
        const double late = ts_ms(&now, &due);
        if (late > 0.0) { /* the radio had nothing to send when this block's slot began */
            p->underruns++;
            if (late > p->worst_late_ms)
                p->worst_late_ms = late;
        }
        if (ts_ms(&now, &room) < 0.0)
            clock_nanosleep(CLOCK_MONOTONIC, TIMER_ABSTIME, &room, NULL); /* iio_buffer_push blocks until there is room (c:2152) */
    }
    int want = p->nkeep == 0;
    for (int i = 0; i < p->nkeep; i++)
        want = want || p->keep[i] == k;
    (void)nsamp;
    if (want && fwrite(iq, 1, p->bytes, p->f) != p->bytes)
        return -1;
    return 0;
}

static int cmp_double(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* -b 8: how many components the shift let saturate (gpsbb_fill_block_ex / the ring's packing kernel counted them); -W: how many
 * the noise did */
/* one -J argument into *e; 0 if it is not well formed (gpsbb_interf_make checks the numbers) */
static int parse_interf(const char *arg, double delt, gpsbb_interf_t *e)
{
    int kind;
    if (!strncmp(arg, "cw,", 3)) {
        kind = GPSBB_INTERF_CW;
        arg += 3;
    } else if (!strncmp(arg, "chirp,", 6)) {
        kind = GPSBB_INTERF_CHIRP;
        arg += 6;
    } else {
        return 0;
    }
    double v[6];
    int n = 0;
    for (;;) {
        char *end = NULL;
        if (n == 6)
            return 0;
        v[n] = strtod(arg, &end);
        if (end == arg || !isfinite(v[n]))
            return 0;
        n++;
        if (*end == 0)
            break;
        if (*end != ',')
            return 0;
        arg = end + 1;
    }
    const int base = kind == GPSBB_INTERF_CW ? 2 : 4;
    if (n != base && n != base + 2)
        return 0;
    const double period = n == base ? 0.0 : v[base], duty = n == base ? 1.0 : v[base + 1];
    if (n != base && !(period > 0.0))
        return 0;
    return gpsbb_interf_make(e, kind, v[0], v[1], kind == GPSBB_INTERF_CW ? 0.0 : v[2], kind == GPSBB_INTERF_CW ? 0.0 : v[3], period,
                             duty, delt) == GPSBB_OK;
}

/* one -M argument, prn,extra_m,atten_db[,phase_cyc[,rate_mps]], into *e; 0 if it is not well formed (gpsfe_set_echoes checks
 * the numbers) */
static int parse_echo(const char *arg, gpsfe_echo_t *e)
{
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int n = 0;
    for (;;) {
        char *end = NULL;
        if (n == 5)
            return 0;
        v[n] = strtod(arg, &end);
        if (end == arg || !isfinite(v[n]))
            return 0;
        n++;
        if (*end == 0)
            break;
        if (*end != ',')
            return 0;
        arg = end + 1;
    }
    if (n < 3 || v[0] < 1.0 || v[0] > 32.0 || v[0] != (double)(int)v[0] || v[1] < 0.0 || v[1] > 30000.0)
        return 0;
    e->prn = (int)v[0];
    e->extra_m = v[1];
    e->atten_db = v[2];
    e->phase_cyc = v[3];
    e->rate_mps = v[4];
    return 1;
}

static void report_clipped(gpsbb_t *bb, int bits, int noise)
{
    uint64_t clipped = 0;
    if (bits == 8 && gpsbb_get_info(bb, GPSBB_INFO_SC8_CLIPPED, &clipped) == GPSBB_OK)
        fprintf(stderr, "8-bit components clipped: %llu\n", (unsigned long long)clipped);
    if (noise && gpsbb_get_info(bb, GPSBB_INFO_NOISE_CLIPPED, &clipped) == GPSBB_OK)
        fprintf(stderr, "noise components clipped: %llu\n", (unsigned long long)clipped);
}

/* -A: the first K blocks of the scenario rendered as a resident batch on `gpu`, measured with the run's noise and emitters from
 * position 0, and the shifts chosen for clip_ppm.  The front end is opened a second time for it: the run's own starts afresh. */
static int agc_choose(const gpsfe_config_t *cfg, int gpu, double delt, long nsamp, long nblocks, unsigned oflags, double clip_ppm,
                      const gpsbb_noise_t *noise, const gpsbb_interf_set_t *interf, const gpsfe_echo_t *echo, int necho, int *a_out,
                      int *q_out)
{
    const int nchan = cfg->max_chan + necho;
    const int K = nblocks < 10 ? (int)(nblocks > 0 ? nblocks : 1) : 10;
    gpsfe_t *fe = NULL;
    gpsbb_t *bb = NULL;
    gpsbb_batch_t *bt = NULL;
    gpsbb_chan_t *ch = malloc((size_t)K * nchan * sizeof *ch);
    gpsbb_level_t *lv = malloc((size_t)K * sizeof *lv);
    int ok = ch && lv && gpsfe_open(cfg, &fe) == GPSFE_OK && gpsfe_set_echoes(fe, echo, necho) == GPSFE_OK;
    int rc = GPSBB_OK;
    if (ok) {
        gpsfe_generate(fe, K, ch);
        rc = gpsbb_create(&bb, gpu);
        if (rc == GPSBB_OK) rc = gpsbb_batch_create(bb, ch, K, nchan, delt, (int)nsamp, GPSBB_CHAIN_CARRIER, &bt);
        if (rc == GPSBB_OK) rc = gpsbb_batch_run(bt, NULL);
        if (rc == GPSBB_OK) rc = gpsbb_sync(bb);
        if (rc == GPSBB_OK) rc = gpsbb_device_level(bb, gpsbb_batch_device_iq(bt), K, (int)nsamp, noise, interf, lv);
        if (rc == GPSBB_OK) {
            rc = gpsbb_level_choose(lv, K, oflags, clip_ppm, a_out, q_out);
            if (rc == 1)
                fprintf(stderr, "agc: even the largest shifts leave more than %g ppm clipped\n", clip_ppm);
            rc = rc < 0 ? rc : GPSBB_OK;
        }
        if (rc == GPSBB_OK) {
            uint64_t c16 = 0, c8 = 0, n = 0;
            const unsigned f = (oflags & GPSBB_OUT_FORMAT_MASK) == (GPSBB_OUT_SC8(0) & GPSBB_OUT_FORMAT_MASK) ? GPSBB_OUT_SC8(*q_out)
                                                                                                              : (oflags & GPSBB_OUT_FORMAT_MASK);
            (void)gpsbb_level_clips(lv, K, *a_out, f, &c16, &c8);
            for (int b = 0; b < K; b++)
                n += 2 * lv[b].n;
            fprintf(stderr, "agc: shift %d, q %d, rms %.1f %.1f, predicted clips %llu %llu of %llu components (%d blocks)\n", *a_out, *q_out,
                    gpsbb_level_rms(lv, K, 0), gpsbb_level_rms(lv, K, 1), (unsigned long long)c16, (unsigned long long)c8,
                    (unsigned long long)n, K);
        } else {
            fprintf(stderr, "ERROR: -A: %s\n", gpsbb_strerror(rc));
        }
    } else {
        fprintf(stderr, "ERROR: -A: cannot prepare the measurement\n");
    }
    if (bt) gpsbb_batch_destroy(bt);
    if (bb) gpsbb_destroy(bb);
    if (fe) gpsfe_close(fe);
    free(ch);
    free(lv);
    return ok && rc == GPSBB_OK;
}

static void usage(void)
{
    fprintf(stderr, "usage: gpsbb-sim -e nav [-l lat,lon,h|-c x,y,z|-u motion.csv] [-t Y/M/D,h:m:s] [-T] [-i] [-3]\n"
                    "                 [-s fs_hz] [-d seconds] [-n samples_per_block] [-N channels] [-g gpu[,gpu...]] [-F] [-G shards [-C [-I]]]\n"
                    "                 [-P usec_per_block] [-Q device_queue_blocks] [-S stats.json] [-k keep,blocks] [-b 1|8|16] [-q shift]\n"
                    "                 [-W cn0_dbhz[,shift]] [-w seed]\n"
                    "                 [-J cw,js_db,f_hz[,period_s,duty]] [-J chirp,js_db,f0_hz,f1_hz,sweep_s[,period_s,duty]] [-j shift]\n"
                    "                 [-M prn,extra_m,atten_db[,phase_cyc[,rate_mps]]]   a multipath echo of satellite prn (up to 8 times;\n"
                    "                                 channels + echoes <= 16): extra path in metres (0..30000), attenuation in dB, reflection\n"
                    "                                 phase in cycles, path rate in m/s\n"
                    "                 [-A clip_ppm]   choose the -W/-j shift and -q from the level of the first second (up to 10 blocks),\n"
                    "                                 once: a later power change shows in the clip counters, not in the scale;\n"
                    "                                 not together with -q, -j or a shift inside -W cn0,shift\n"
                    "                 [-D decim[,ntaps[,cutoff[,atten_db]]]]   render at -s times decim (1..16), band-limit with a Kaiser-windowed\n"
                    "                                 sinc (default 8 * decim + 1 taps, cutoff 0.8 of the file's Nyquist rate, 60 dB) and write\n"
                    "                                 every decim-th sample at -s; -W and -J act at the rendered rate; not with -A -P -k -S -R -G\n"
                    "                 -o out.bin\n");
}

int main(int argc, char **argv)
{
    /* This program runs host-bound rings, one handle per shard: more streams than the runtime's default of four hardware
     * queues (three per handle, a copy stream each, the null stream), and streams that share a queue run one
     * after the other.  This is the host's call (before its first HIP call); the library does not touch the environment. */
    setenv("GPU_MAX_HW_QUEUES", "12", 0);
    gpsfe_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.pos[0] = 35.681298; /* default static location: Tokyo (c:2266-2268) */
    cfg.pos[1] = 139.766247;
    cfg.pos[2] = 10.0;
    cfg.max_chan = 12; /* MAX_CHAN h:21 */
    long fs_hz = 3000000; /* TX_SAMPLE_FREQ c:43 */
    long nsamp = 300000;  /* NUM_SAMPLES c:44 */
    double duration = 1.0;
    int gpu = 0, opt, fast = 0, no_register = 0, nshards = 0, ndev = 0, interleaved = 0, contiguous = 0;
    int16_t *iq_registered = NULL;
    int devs[GPSBB_NODE_MAX_SHARDS];
    struct paced_sink paced;
    memset(&paced, 0, sizeof paced);
    paced.queue = 4; /* libiio's default number of kernel buffers */
    const char *stats_path = NULL;
    const char *out_path = NULL;
    int bits = 16, shift = 5, shift_given = 0;
    const char *agc_arg = NULL;
    const char *decim_arg = NULL;
    const char *noise_arg = NULL;
    unsigned long long noise_seed = 1;
    const char *interf_arg[GPSBB_INTERF_MAX + 1];
    int ninterf = 0;
    const char *interf_shift_arg = NULL;
    const char *echo_arg[GPSFE_MAX_ECHOES + 1];
    int nechoarg = 0;

    while ((opt = getopt(argc, argv, "e:u:c:l:s:Tt:in:N:d:o:g:3FG:P:S:k:Q:ICRb:q:W:w:J:j:A:M:D:")) != -1) {
        switch (opt) {
        case 'e': cfg.navfile = optarg; break;
        case 'u': cfg.motion_file = optarg; break;
        case 'c':
        case 'l':
            cfg.use_ecef = opt == 'c';
            if (sscanf(optarg, "%lf,%lf,%lf", &cfg.pos[0], &cfg.pos[1], &cfg.pos[2]) != 3) {
                fprintf(stderr, "ERROR: -%c wants three comma-separated numbers\n", opt);
                return 1;
            }
            break;
        case 's':
            fs_hz = atol(optarg);
            if (fs_hz < 1000000) { /* c:2326 */
                fprintf(stderr, "ERROR: Invalid sampling frequency.\n");
                return 1;
            }
            break;
        case 'T': cfg.time_overwrite = 1; break;
        case 't':
            cfg.have_start = 1;
            if (sscanf(optarg, "%d/%d/%d,%d:%d:%lf", &cfg.y, &cfg.m, &cfg.d, &cfg.hh, &cfg.mm, &cfg.sec) != 6) {
                fprintf(stderr, "ERROR: -t wants YYYY/MM/DD,hh:mm:ss\n");
                return 1;
            }
            break;
        case 'i': cfg.iono_disable = 1; break;
        case '3': cfg.rinex3 = 1; break; /* the reference declares -3 with an argument (c:2296); here it is a flag */
        case 'n': nsamp = atol(optarg); break;
        case 'N': cfg.max_chan = atoi(optarg); break;
        case 'd': duration = atof(optarg); break;
        case 'o': out_path = optarg; break;
        case 'g': /* one ordinal, or the list of the node driver's shards */
            ndev = 0;
            for (char *t = strtok(optarg, ","); t && ndev < GPSBB_NODE_MAX_SHARDS; t = strtok(NULL, ","))
                devs[ndev++] = atoi(t);
            gpu = ndev ? devs[0] : 0;
            break;
        case 'G': nshards = atoi(optarg); break;
        case 'I': interleaved = 1; break;
        case 'C': contiguous = 1; break; /* (with -I alone: the whole sequence up front as well: GPSBB_NODE_INTERLEAVED) */
        case 'P': paced.period_ns = atol(optarg) * 1000L; break;
        case 'S': stats_path = optarg; break;
        case 'Q': paced.queue = atoi(optarg) > 0 ? atoi(optarg) : 1; break;
        case 'k':
            for (char *t = strtok(optarg, ","); t && paced.nkeep < 64; t = strtok(NULL, ","))
                paced.keep[paced.nkeep++] = atol(t);
            break;
        case 'F': fast = 1; break;
        case 'R': no_register = 1; break; /* the drop-in call copies into iq_buff instead of rendering straight into it */
        case 'b': bits = atoi(optarg); break;
        case 'q': shift = atoi(optarg); shift_given = 1; break;
        case 'A': agc_arg = optarg; break;
        case 'D': decim_arg = optarg; break;
        case 'W': noise_arg = optarg; break;
        case 'w': noise_seed = strtoull(optarg, NULL, 0); break;
        case 'J':
            if (ninterf <= GPSBB_INTERF_MAX)
                interf_arg[ninterf < GPSBB_INTERF_MAX ? ninterf : GPSBB_INTERF_MAX] = optarg;
            ninterf++;
            break;
        case 'j': interf_shift_arg = optarg; break;
        case 'M':
            echo_arg[nechoarg < GPSFE_MAX_ECHOES ? nechoarg : GPSFE_MAX_ECHOES] = optarg;
            nechoarg++;
            break;
        default: usage(); return 1;
        }
    }
    if (!cfg.navfile || !out_path || (bits != 1 && bits != 8 && bits != 16) || shift < 0 || shift > 15) {
        usage();
        return 1;
    }
    double agc_ppm = 0.0;
    if (agc_arg) {
        char *end = NULL;
        agc_ppm = strtod(agc_arg, &end);
        if (end == agc_arg || *end != 0 || !(agc_ppm >= 0.0) || !isfinite(agc_ppm) || shift_given || interf_shift_arg ||
            (noise_arg && strchr(noise_arg, ','))) {
            fprintf(stderr, "ERROR: -A wants a clip budget in ppm (>= 0) and chooses the shifts itself: not with -q, -j or -W cn0,shift\n");
            usage();
            return 1;
        }
    }
    if (nsamp == 0)
        nsamp = fs_hz / 10;
    /* -D: the filter, checked before anything is opened; from here on fs_hz and nsamp are the render's, nsamp_out the file's */
    const long nsamp_out = nsamp;
    int decim = 0;
    gpsbb_fir_t fir;
    memset(&fir, 0, sizeof fir);
    if (decim_arg) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        int n = 0, ok = 1;
        for (const char *arg = decim_arg; ok;) {
            char *end = NULL;
            ok = n < 4;
            if (!ok)
                break;
            v[n] = strtod(arg, &end);
            ok = end != arg && isfinite(v[n]) && (*end == 0 || *end == ',');
            n++;
            if (!ok || *end == 0)
                break;
            arg = end + 1;
        }
        ok = ok && v[0] >= 1.0 && v[0] <= 16.0 && v[0] == (double)(int)v[0] && (n < 2 || (v[1] >= 1.0 && v[1] <= 1e6 && v[1] == (double)(int)v[1]));
        decim = ok ? (int)v[0] : 0;
        if (!ok || gpsbb_fir_make(&fir, n >= 2 ? (int)v[1] : 8 * decim + 1, decim, v[2], v[3]) != GPSBB_OK) {
            fprintf(stderr, "ERROR: -D wants decim[,ntaps[,cutoff[,atten_db]]]: decim 1..16, ntaps 1..%d, a cutoff in (0, 1], at most 180 dB\n",
                    GPSBB_FIR_MAX_TAPS);
            return 1;
        }
        int refused = 0;
        if (agc_arg) refused += fprintf(stderr, "ERROR: -D not together with -A: -A measures the level before the filter\n") > 0;
        if (paced.period_ns) refused += fprintf(stderr, "ERROR: -D not together with -P: the filter's path is not paced\n") > 0;
        if (paced.nkeep) refused += fprintf(stderr, "ERROR: -D not together with -k: the filter's path writes every block\n") > 0;
        if (nshards > 0) refused += fprintf(stderr, "ERROR: -D not together with -G: the node driver has no filter stage\n") > 0;
        if (stats_path || no_register)
            refused += fprintf(stderr, "ERROR: -D not together with -S or -R: they belong to the block-by-block hand-off, which has no filter stage\n") > 0;
        if (refused)
            return 1;
        fs_hz *= decim;
        nsamp *= decim;
    }
    /* the output format, the same bits on every path (fill, stream, node) */
    unsigned oflags = bits == 8 ? GPSBB_OUT_SC8(shift) : (bits == 1 ? GPSBB_OUT_SC1 : GPSBB_OUT_SC16);
    const long obytes = gpsbb_out_bytes(oflags, nsamp_out);
    if (obytes < 0) {
        fprintf(stderr, "ERROR: -b %d needs a block of a multiple of 4 samples (-n)\n", bits);
        return 1;
    }
    const double delt = 1.0 / (double)fs_hz; /* c:2397 */
    const long nblocks = (long)(duration * 10.0 + 0.5);
    /* -W: the noise, checked before anything is opened; block b starts at stream position b * nsamp on every path */
    gpsbb_noise_t nz;
    memset(&nz, 0, sizeof nz);
    const gpsbb_noise_t *noise = NULL;
    if (noise_arg) {
        char *end = NULL;
        const double cn0 = strtod(noise_arg, &end);
        int nshift = 0, ok = end != noise_arg && isfinite(cn0);
        if (ok && *end == ',') {
            char *e2 = NULL;
            const long v = strtol(end + 1, &e2, 10);
            ok = e2 != end + 1 && *e2 == 0 && v >= 0 && v <= 7;
            nshift = (int)v;
        } else {
            ok = ok && *end == 0;
        }
        nz.sigma = ok ? gpsbb_noise_sigma(cn0, 1.0, delt) : NAN;
        if (!ok || !(nz.sigma > 0.0) || nz.sigma > 1048576.0) {
            fprintf(stderr, "ERROR: -W wants a finite C/N0 in dB-Hz and a shift of 0..7 (cn0[,shift]), sigma <= 2^20\n");
            return 1;
        }
        nz.seed = noise_seed;
        nz.shift = nshift;
        noise = &nz;
        fprintf(stderr, "noise: C/N0 %.2f dB-Hz at gain 1.0, sigma %.1f LSB per component, shift %d, seed %llu\n", cn0, nz.sigma,
                nshift, (unsigned long long)noise_seed);
    }
    /* -J: the interference, checked here as well; the noise's position and shift */
    gpsbb_interf_set_t jset;
    memset(&jset, 0, sizeof jset);
    const gpsbb_interf_set_t *interf = NULL;
    if (ninterf > 0 || interf_shift_arg) {
        int ok = ninterf >= 1 && ninterf <= GPSBB_INTERF_MAX;
        for (int k = 0; ok && k < ninterf; k++)
            ok = parse_interf(interf_arg[k], delt, &jset.e[k]);
        jset.n = ninterf;
        jset.shift = noise ? nz.shift : 0;
        if (ok && interf_shift_arg) {
            char *e2 = NULL;
            const long v = strtol(interf_shift_arg, &e2, 10);
            ok = e2 != interf_shift_arg && *e2 == 0 && v >= 0 && v <= 7 && (!noise || v == nz.shift);
            jset.shift = (int)v;
        }
        if (!ok) {
            fprintf(stderr, "ERROR: -J wants cw,js_db,f_hz or chirp,js_db,f0_hz,f1_hz,sweep_s, each with an optional ,pulse_period_s,duty, "
                            "at most %d times: |f| at most half the sampling rate, a sweep of 2 samples or more, a duty in (0, 1]; "
                            "-j a shift of 0..7 that goes with -J (and equals -W's)\n", GPSBB_INTERF_MAX);
            return 1;
        }
        interf = &jset;
        fprintf(stderr, "interference: %d emitter%s, shift %d\n", jset.n, jset.n == 1 ? "" : "s", jset.shift);
    }

    /* -M: the echoes, checked here as well */
    gpsfe_echo_t echo[GPSFE_MAX_ECHOES];
    memset(echo, 0, sizeof echo);
    {
        int ok = nechoarg == 0 || (nechoarg <= GPSFE_MAX_ECHOES && cfg.max_chan >= 1 && cfg.max_chan + nechoarg <= GPSBB_MAX_CHAN);
        for (int k = 0; ok && k < nechoarg; k++)
            ok = parse_echo(echo_arg[k], &echo[k]);
        if (!ok) {
            fprintf(stderr, "ERROR: -M wants prn,extra_m,atten_db[,phase_cyc[,rate_mps]], at most %d times and channels + echoes <= %d: "
                            "a prn of 1..32, an extra path of 0..30000 m\n", GPSFE_MAX_ECHOES, GPSBB_MAX_CHAN);
            return 1;
        }
    }
    const int necho = nechoarg;

    if (agc_arg) {
        /* -A: both shifts from the level of the first blocks; from here on the run is the one of the explicit options */
        int a = 0, q = 0;
        if (!agc_choose(&cfg, nshards > 0 && ndev > 0 ? devs[0] : gpu, delt, nsamp, nblocks, oflags, agc_ppm, noise, interf, echo, necho, &a, &q))
            return 1;
        nz.shift = a;
        jset.shift = a;
        if (bits == 8) {
            shift = q;
            oflags = GPSBB_OUT_SC8(shift);
        }
    }
    gpsfe_t *fe = NULL;
    int rc = gpsfe_open(&cfg, &fe);
    if (rc != GPSFE_OK) {
        fprintf(stderr, "ERROR: %s\n", gpsfe_strerror(rc));
        return 1;
    }
    if (necho > 0 && (rc = gpsfe_set_echoes(fe, echo, necho)) != GPSFE_OK) {
        fprintf(stderr, "ERROR: -M: %s\n", gpsfe_strerror(rc));
        return 1;
    }
    const int nchan = gpsfe_block_chans(fe); /* the channel count of every call below: the satellites' slots and the echoes' */
    if (necho > 0)
        fprintf(stderr, "echoes: %d, %d descriptors per block\n", necho, nchan);
    if (nshards > 0) {
        /* the whole descriptor sequence first (the host range solver runs ahead of everything: 296 bytes per block-channel),
         * then N time shards on N handles into one output */
        if (nshards > GPSBB_NODE_MAX_SHARDS || (ndev > 1 && ndev != nshards) || nblocks < 1) {
            fprintf(stderr, "ERROR: -G wants 1..%d shards and as many -g ordinals\n", GPSBB_NODE_MAX_SHARDS);
            return 1;
        }
        for (int g = 0; g < nshards; g++)
            devs[g] = ndev > 1 ? devs[g] : (ndev == 1 && nshards == 1 ? devs[0] : (ndev == 1 ? devs[0] + g : g));
        /* Default: the stream as the reference makes it, incrementally (gpsbb_node_begin / _feed / _end): the front end generates
         * a few slots' worth of descriptors, feeds them, and goes round again while the GPUs render — it runs one queue ahead of
         * the rings, and the memory this takes does not depend on -d.  -C: contiguous time shards (BASELINE configs[4]'s layout),
         * which need the whole descriptor sequence up front (296 bytes per block and channel). */
        const int bps = nblocks < 16 ? (int)nblocks : 16;
        contiguous = contiguous || interleaved;
        const long chunk = contiguous ? nblocks : (long)bps * nshards * 2;
        gpsbb_chan_t *all = malloc((size_t)chunk * nchan * sizeof *all);
        FILE *fo = strcmp(out_path, "-") ? fopen(out_path, "wb") : stdout;
        if (!all || !fo) {
            fprintf(stderr, "ERROR: cannot allocate the descriptors / open %s\n", out_path);
            return 1;
        }
        struct node_out o = {fo, -1, (size_t)obytes};
        unsigned nflags = interleaved ? GPSBB_NODE_INTERLEAVED : 0u; /* -C -I: the slots go round the GPUs (an ordered output scales) */
        if (fo != stdout && ftruncate(fileno(fo), (off_t)nblocks * obytes) == 0) {
            o.fd = fileno(fo); /* a regular file: blocks are placed by index as they complete, from every shard at once */
            nflags |= GPSBB_NODE_INDEXED | GPSBB_NODE_CONCURRENT;
        }
        gpsbb_node_config_t nc = {nshards, devs, nchan, delt, (int)nsamp, bps, 3, nflags | oflags};
        gpsbb_node_t *node = NULL;
        gpsbb_node_stats_t ns;
        rc = gpsbb_node_create(&node, &nc);
        if (rc == GPSBB_OK && noise)
            rc = gpsbb_node_set_noise(node, noise);
        if (rc == GPSBB_OK && interf)
            rc = gpsbb_node_set_interf(node, interf);
        if (rc == GPSBB_OK && contiguous) {
            gpsfe_generate(fe, (int)nblocks, all);
            rc = gpsbb_node_run(node, all, nblocks, node_sink, &o, &ns);
        } else if (rc == GPSBB_OK) {
            rc = gpsbb_node_begin(node, node_sink, &o);
            for (long done = 0; rc == GPSBB_OK && done < nblocks; done += chunk) { /* while (!plutotx.exit), c:2655 */
                const long nb = nblocks - done < chunk ? nblocks - done : chunk;
                gpsfe_generate(fe, (int)nb, all);                  /* c:2656-2687 (+ c:2764-2805) */
                rc = gpsbb_node_feed(node, all, nb);
            }
            const int rc_end = gpsbb_node_end(node, &ns);
            rc = rc == GPSBB_OK || rc == GPSBB_E_STATE ? rc_end : rc;
        }
        if (rc != GPSBB_OK)
            fprintf(stderr, "ERROR: node driver: %s\n", gpsbb_strerror(rc));
        else
            for (int g = 0; g < ns.nshards; g++)
                fprintf(stderr, "shard %d: gpu %d (numa node %d, %d cpus), blocks %ld..%ld, seed %.3f s, busy %.3f s\n", g,
                        ns.shard[g].device, ns.shard[g].numa_node, ns.shard[g].cpus_bound, ns.shard[g].first_block,
                        ns.shard[g].first_block + ns.shard[g].nblocks, ns.shard[g].seed_seconds, ns.shard[g].busy_seconds);
        gpsbb_node_destroy(node);
        free(all);
        if (fo != stdout)
            fclose(fo);
        else
            fflush(fo);
        gpsfe_close(fe);
        if (rc == GPSBB_OK)
            fprintf(stderr, "%ld blocks of %ld samples written\n", nblocks, nsamp);
        return rc == GPSBB_OK ? 0 : 1;
    }
    gpsbb_t *bb = NULL;
    rc = gpsbb_create(&bb, gpu);
    if (rc != GPSBB_OK) {
        fprintf(stderr, "ERROR: gpsbb_create: %s\n", gpsbb_strerror(rc));
        return 1;
    }
    FILE *fout = strcmp(out_path, "-") ? fopen(out_path, "wb") : stdout;
    if (!fout) {
        fprintf(stderr, "ERROR: cannot open %s\n", out_path);
        return 1;
    }
    if (decim) {
        /* -D: render at the input rate into a device-only ring, filter each popped slot on the device with the history carried,
         * pack what is left and write it.  The decimated slot needs device memory and the ABI hands out none by itself: it is
         * the output buffer of a resident batch of the slot's shape at the file's rate, run once and then only written to. */
        const int bps = nblocks < 4 ? (int)(nblocks > 0 ? nblocks : 1) : 4, depth = 3;
        gpsbb_stream_t *st = NULL;
        gpsbb_batch_t *room = NULL;
        gpsfe_t *fe2 = NULL;
        gpsbb_chan_t *slot = malloc((size_t)bps * nchan * sizeof *slot);
        unsigned char *host = malloc((size_t)bps * (size_t)obytes);
        int16_t hist[2 * GPSBB_FIR_MAX_TAPS];
        memset(hist, 0, sizeof hist);
        int16_t *d_out = NULL;
        rc = slot && host ? GPSBB_OK : GPSBB_E_NOMEM;
        if (rc == GPSBB_OK && (gpsfe_open(&cfg, &fe2) != GPSFE_OK || gpsfe_set_echoes(fe2, echo, necho) != GPSFE_OK))
            rc = GPSBB_E_STATE;
        if (rc == GPSBB_OK) {
            gpsfe_generate(fe2, bps, slot);
            rc = gpsbb_batch_create(bb, slot, bps, nchan, delt * decim, (int)nsamp_out, GPSBB_CHAIN_CARRIER, &room);
        }
        if (rc == GPSBB_OK) rc = gpsbb_batch_run(room, NULL);
        if (rc == GPSBB_OK) rc = gpsbb_sync(bb);
        if (rc == GPSBB_OK && !(d_out = gpsbb_batch_device_iq(room))) rc = GPSBB_E_STATE;
        if (rc == GPSBB_OK)
            rc = gpsbb_stream_create(bb, nchan, delt, (int)nsamp, bps, depth, GPSBB_CHAIN_CARRIER | GPSBB_STREAM_DEVICE_ONLY, &st);
        long pushed = 0, written = 0;
        uint64_t pos = 0, clipped = 0;
        while (rc == GPSBB_OK && written < nblocks) {
            while (rc == GPSBB_OK && pushed < nblocks && gpsbb_stream_pending(st) < depth) {
                gpsfe_generate(fe, bps, slot); /* a short last slot is padded with blocks that are generated but not written */
                rc = gpsbb_stream_push(st, slot);
                pushed += bps;
            }
            const int16_t *d_iq = NULL;
            if (rc == GPSBB_OK)
                rc = gpsbb_stream_pop(st, &d_iq, NULL);
            if (rc == GPSBB_OK) {
                uint64_t c = 0;
                nz.sample0 = jset.sample0 = pos;
                rc = gpsbb_device_fir(bb, d_iq, (long)bps * nsamp, noise, interf, &fir, hist, hist, d_out, &c);
                pos += (uint64_t)bps * (uint64_t)nsamp;
                clipped += c;
            }
            if (rc == GPSBB_OK)
                rc = gpsbb_device_pack(bb, d_out, bps, (int)nsamp_out, oflags, host);
            if (rc == GPSBB_OK) {
                const long n = nblocks - written < bps ? nblocks - written : bps;
                if (fwrite(host, (size_t)obytes, (size_t)n, fout) != (size_t)n)
                    rc = GPSBB_E_STATE;
                written += n;
            }
        }
        if (rc != GPSBB_OK)
            fprintf(stderr, "ERROR: -D: %s\n", gpsbb_strerror(rc));
        fprintf(stderr, "filter: %d taps, decimation %d, shift %d; components clipped: %llu\n", fir.ntaps, fir.decim, fir.shift,
                (unsigned long long)clipped);
        if (st) gpsbb_stream_destroy(st);
        if (room) gpsbb_batch_destroy(room);
        report_clipped(bb, bits, 0);
        free(slot);
        free(host);
        if (fout != stdout)
            fclose(fout);
        gpsbb_destroy(bb);
        if (fe2) gpsfe_close(fe2);
        gpsfe_close(fe);
        fprintf(stderr, "%ld blocks of %ld samples written\n", written, nsamp_out);
        return rc == GPSBB_OK ? 0 : 1;
    }
    if (fast) {
        /* offline generation: slots of up to 16 blocks through the ring, three in flight */
        const int bps = nblocks < 16 ? (int)(nblocks > 0 ? nblocks : 1) : 16, depth = 3;
        gpsbb_stream_t *st = NULL;
        gpsbb_chan_t *slot = malloc((size_t)bps * nchan * sizeof *slot);
        rc = slot ? gpsbb_stream_create(bb, nchan, delt, (int)nsamp, bps, depth, GPSBB_CHAIN_CARRIER | oflags, &st) : GPSBB_E_NOMEM;
        if (rc == GPSBB_OK && noise)
            rc = gpsbb_stream_set_noise(st, noise); /* from block 0: every push moves the position on by its blocks */
        if (rc == GPSBB_OK && interf)
            rc = gpsbb_stream_set_interf(st, interf);
        long pushed = 0, written = 0;
        while (rc == GPSBB_OK && slot && written < nblocks) {
            while (rc == GPSBB_OK && pushed < nblocks && gpsbb_stream_pending(st) < depth) {
                /* a short last slot is padded with blocks that are generated but not written */
                gpsfe_generate(fe, bps, slot);
                rc = gpsbb_stream_push(st, slot);
                pushed += bps;
            }
            const int16_t *iq = NULL;
            if (rc == GPSBB_OK)
                rc = gpsbb_stream_pop(st, &iq, NULL);
            if (rc == GPSBB_OK) {
                const long n = nblocks - written < bps ? nblocks - written : bps;
                if (fwrite(iq, (size_t)obytes, (size_t)n, fout) != (size_t)n)
                    rc = GPSBB_E_STATE;
                written += n;
            }
        }
        if (rc != GPSBB_OK)
            fprintf(stderr, "ERROR: streaming: %s\n", gpsbb_strerror(rc));
        if (st)
            gpsbb_stream_destroy(st);
        report_clipped(bb, bits, noise != NULL || interf != NULL);
        free(slot);
        if (fout != stdout)
            fclose(fout);
        gpsbb_destroy(bb);
        gpsfe_close(fe);
        fprintf(stderr, "%ld blocks of %ld samples written\n", written, nsamp);
        return rc == GPSBB_OK ? 0 : 1;
    }

    gpsbb_tx_t *tx = NULL;
    paced.f = fout;
    paced.bytes = (size_t)obytes;
    double *lat_ms = calloc((size_t)(nblocks > 0 ? nblocks : 1), sizeof *lat_ms);
    if (gpsbb_tx_create(&tx, (size_t)nsamp, paced_push, &paced) != 0 || !lat_ms) {
        fprintf(stderr, "ERROR: cannot start the TX surface\n");
        return 1;
    }

    fprintf(stderr, "PRN   Az    El     Range     Iono\n"); /* the table the reference prints, c:2634-2639 */
    for (int i = 0; i < cfg.max_chan; i++) {
        int prn;
        double az, el, range, iono;
        gpsfe_channel_info(fe, i, &prn, &az, &el, &range, &iono);
        if (prn > 0)
            fprintf(stderr, "%02d %6.1f %5.1f %11.1f %5.1f\n", prn, az, el, range, iono);
    }

    gpsbb_chan_t ch[GPSBB_MAX_CHAN];
    gpsbb_chan_state_t st[GPSBB_MAX_CHAN];
    long blk;
    for (blk = 0; blk < nblocks; blk++) { /* while (!plutotx.exit), c:2655 */
        gpsfe_next_block(fe, ch);                                   /* c:2656-2687 (+ c:2764-2805) */
        if (blk == 0) {
            /* The first two calls on a handle pay for what every later one finds in place (code objects loaded, scratch
             * and both table sets allocated: 18 and 10 ms against 0.3): render the first block twice into a scratch buffer
             * before the consumer's clock starts.  A fill has no side effects besides its outputs ... */
            int16_t *scratch = malloc((size_t)nsamp * 4);
            for (int w = 0; scratch && w < 2; w++)
                (void)gpsbb_fill_block(bb, ch, nchan, delt, (int)nsamp, scratch, NULL);
            free(scratch);
            /* ... besides the handle's hazard counters: block 0 must count once in the note at the end, not three times */
            gpsbb_hazards_t warm;
            (void)gpsbb_get_hazards(bb, &warm, 1);
        }
        int16_t *iq = gpsbb_tx_begin(tx);                           /* c:2689 */
        if (blk == 0 && !no_register && gpsbb_host_register(bb, iq, (size_t)nsamp * 4) == GPSBB_OK)
            iq_registered = iq; /* iq_buff is one allocation for the run (c:2604): rendered into directly from here on */
        struct timespec ta, tb;
        clock_gettime(CLOCK_MONOTONIC, &ta);
        if (interf) {
            nz.sample0 = jset.sample0 = (uint64_t)blk * (uint64_t)nsamp;
            rc = gpsbb_fill_block_impair(bb, ch, nchan, delt, (int)nsamp, oflags, noise, &jset, iq, st);
        } else if (noise) {
            nz.sample0 = (uint64_t)blk * (uint64_t)nsamp;
            rc = gpsbb_fill_block_noise(bb, ch, nchan, delt, (int)nsamp, oflags, &nz, iq, st);
        } else {
            rc = gpsbb_fill_block_ex(bb, ch, nchan, delt, (int)nsamp, oflags, iq, st); /* replaces c:2690-2756 */
        }
        clock_gettime(CLOCK_MONOTONIC, &tb);
        lat_ms[blk] = ts_ms(&tb, &ta);
        if (rc != GPSBB_OK) { /* the buffer holds no valid block: it must not reach the sink */
            gpsbb_tx_cancel(tx);
            fprintf(stderr, "ERROR: gpsbb_fill_block_ex: %s\n", gpsbb_strerror(rc));
            break;
        }
        const int stopped = gpsbb_tx_end(tx);                       /* c:2757-2759 */
        gpsfe_feed_back(fe, st); /* the loop's in-place update of chan[i].carr_phase */
        if (stopped)
            break;
    }
    if (iq_registered)
        (void)gpsbb_host_unregister(bb, iq_registered); /* before the buffer is freed (c:2815) */
    gpsbb_tx_destroy(tx);
    if (fout != stdout)
        fclose(fout);
    if (stats_path && blk > 0) {
        /* the drop-in call's latency over the whole run, and what the paced consumer saw */
        /* which blocks were slow (before the sort loses the order): the first 32 above 2 ms */
        char slow[2048];
        size_t so = 0;
        int nslow = 0;
        slow[0] = 0;
        for (long i = 0; i < blk; i++)
            if (lat_ms[i] > 2.0) {
                if (nslow < 32 && so + 40 < sizeof slow)
                    so += (size_t)snprintf(slow + so, sizeof slow - so, "%s[%ld, %.2f]", nslow ? ", " : "", i, lat_ms[i]);
                nslow++;
            }
        qsort(lat_ms, (size_t)blk, sizeof *lat_ms, cmp_double);
        double sum = 0.0;
        for (long i = 0; i < blk; i++)
            sum += lat_ms[i];
        FILE *sf = fopen(stats_path, "w");
        if (sf) {
            fprintf(sf, "{\"blocks\": %ld, \"nsamp\": %ld, \"channels\": %d, \"fs_hz\": %ld, \"period_us\": %.1f, \"device_queue_blocks\": %d, "
                        "\"fill_block_ms\": {\"mean\": %.4f, \"p50\": %.4f, \"p90\": %.4f, \"p99\": %.4f, \"p999\": %.4f, \"max\": %.4f}, "
                        "\"underruns\": %ld, \"worst_late_ms\": %.4f, \"delivered\": %ld, \"blocks_over_2ms\": %d, \"first_slow_blocks\": [%s]}\n",
                    blk, nsamp, nchan, fs_hz, (double)paced.period_ns / 1e3, paced.queue, sum / (double)blk, lat_ms[blk / 2],
                    lat_ms[(long)((double)blk * 0.9)], lat_ms[(long)((double)blk * 0.99)], lat_ms[(long)((double)blk * 0.999)],
                    lat_ms[blk - 1], paced.underruns, paced.worst_late_ms, paced.seen, nslow, slow);
            fclose(sf);
        }
    }
    free(lat_ms);
    gpsbb_hazards_t hz;
    if (gpsbb_get_hazards(bb, &hz, 0) == GPSBB_OK && (hz.itable_512 || hz.dwrd_oob))
        fprintf(stderr, "note: latent out-of-bounds cases of the reference hit: table %llu, nav words %llu\n",
                (unsigned long long)hz.itable_512, (unsigned long long)hz.dwrd_oob);
    report_clipped(bb, bits, noise != NULL || interf != NULL);
    gpsbb_destroy(bb);
    gpsfe_close(fe);
    fprintf(stderr, "%ld blocks of %ld samples written\n", blk, nsamp);
    return rc == GPSBB_OK ? 0 : 1;
}
