/*
 * The host front end (pluto-gps-sim_amd/host/gpsfe.c) on navigation and motion files that are damaged, on a machine without
 * a GPU: every file of a directory goes through gpsfe_open and the calls that follow it, each in a child process of its own
 * with a time limit of its own, so that a hang or a crash costs one case.  tests/test_frontend_malformed.py writes the
 * corpus of tests/rinex_mutants.py to a directory and runs this program over it, built twice from gpsfe.c itself (not from
 * libgpsfe.so): with the product's flags, and under the host sanitizers.
 *   cc -std=c11 -O2 -ffp-contract=off -fno-builtin -D_GNU_SOURCE -Iinclude tools/fe_asan.c pluto-gps-sim_amd/host/gpsfe.c \
 *      -o fe_plain -lm -lz -lpthread
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -fno-builtin -D_GNU_SOURCE \
 *      -Iinclude tools/fe_asan.c pluto-gps-sim_amd/host/gpsfe.c -o fe_asan -lm -lz -lpthread
 *   ./fe_asan CASEDIR GOODNAV LIMIT_MS
 * A case is a file of CASEDIR: NAME.n2 a navigation file for the RINEX 2 reader, NAME.n3 one for the RINEX 3 reader, NAME.csv
 * a motion file (read beside GOODNAV, a sound RINEX 2 file).  One line per case on stdout, in the order of the names:
 *   NAME open=RC sets=N valid=A,B,.. openT=RC openR=RC end=HOW
 * RC is gpsfe_open's return: plain, with -T and a start time, and with a start time 20 s before the golden files' second set
 * becomes current (the roll-over to the next set, c:2776-2790, then happens inside the run); sets/valid are gpsfe_eph_sets
 * of the plain open (sets=- when it failed); HOW is "ok", "signal N", "timeout", "baddesc: ..." (a descriptor that is not fit to render, or one that differs
 * between one thread and four) or "exit N" (not this program's own exit: a sanitizer's report, which goes to stderr after a
 * line "== NAME").  Exit status 1 if any case ended other than "ok".
 * Never loaded into Python, never run on a GPU: nothing here makes a HIP call.
 */
#include <dirent.h>
#include <math.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <sys/wait.h>
#include <unistd.h>

#include "gpsfe.h"

/* leak checking needs ptrace, which a build machine may not grant; every other check stays on */
const char *__asan_default_options(void) { return "detect_leaks=0"; }

#define MAX_CHAN 12
#define N_GEN 313 /* 3 + 310 blocks: crosses the 30 s maintenance at block 299 */
#define EXIT_BADDESC 3

static char why[256];

/* what the GPU side's contract (include/gpsbb.h) asks of a descriptor */
static int desc_ok(const gpsbb_chan_t *d, int n, const char *leg)
{
    for (int i = 0; i < n; i++) {
        const gpsbb_chan_t *c = &d[i];
        const char *bad = NULL;
        if (!isfinite(c->f_carr) || !isfinite(c->f_code) || !isfinite(c->carr_phase) || !isfinite(c->code_phase) || !isfinite(c->gain))
            bad = "a field is not finite";
        else if (c->prn < 0 || c->prn > 32)
            bad = "prn outside 0..32";
        else if (c->iword < 0 || c->iword > 59)
            bad = "iword outside 0..59";
        else if (c->ibit < 0 || c->ibit > 29 || c->icode < 0 || c->icode > 19)
            bad = "ibit or icode out of range";
        else if (c->prn > 0 && !(c->f_code > 0.0))
            bad = "f_code <= 0 on an active channel";
        if (bad) {
            snprintf(why, sizeof why, "%s: %s (desc %d: prn %d iword %d f_code %g f_carr %g code_phase %g gain %g)", leg, bad, i,
                     c->prn, c->iword, c->f_code, c->f_carr, c->code_phase, c->gain);
            return 0;
        }
    }
    return 1;
}

/* one configuration, start to end.  Returns gpsfe_open's code; *bad is set on a descriptor that fails. */
static int run_config(const gpsfe_config_t *cfg, int *bad, char *sets, size_t sets_cap)
{
    static gpsbb_chan_t seq[N_GEN * GPSBB_MAX_CHAN], par[N_GEN * GPSBB_MAX_CHAN], blk[GPSBB_MAX_CHAN];
    gpsfe_t *fe = NULL;
    int rc = gpsfe_open(cfg, &fe);
    if (rc != GPSFE_OK)
        return rc;
    if (sets) {
        int nv[16] = {0};
        const int ns = gpsfe_eph_sets(fe, nv, 16);
        int at = snprintf(sets, sets_cap, "sets=%d valid=", ns);
        for (int s = 0; s < ns && s < 16 && at < (int)sets_cap; s++)
            at += snprintf(sets + at, sets_cap - (size_t)at, "%s%d", s ? "," : "", nv[s]);
    }
    /* three blocks one by one, then 310 on one thread */
    for (int b = 0; b < 3 && !*bad; b++)
        if (gpsfe_next_block(fe, seq + b * MAX_CHAN) != GPSFE_OK || !desc_ok(seq + b * MAX_CHAN, MAX_CHAN, "next_block"))
            *bad = 1;
    gpsfe_set_threads(fe, 1);
    if (!*bad && (gpsfe_generate(fe, N_GEN - 3, seq + 3 * MAX_CHAN) != GPSFE_OK || !desc_ok(seq, N_GEN * MAX_CHAN, "generate, 1 thread")))
        *bad = 1;
    gpsfe_close(fe);
    if (*bad)
        return rc;
    /* the same blocks on four threads */
    if (gpsfe_open(cfg, &fe) != GPSFE_OK) {
        snprintf(why, sizeof why, "a second gpsfe_open of the same file failed");
        *bad = 1;
        return rc;
    }
    gpsfe_set_threads(fe, 4);
    if (gpsfe_generate(fe, N_GEN, par) != GPSFE_OK || !desc_ok(par, N_GEN * MAX_CHAN, "generate, 4 threads"))
        *bad = 1;
    else if (memcmp(seq, par, sizeof(gpsbb_chan_t) * N_GEN * MAX_CHAN) != 0) {
        snprintf(why, sizeof why, "generate on 4 threads differs from 1 thread");
        *bad = 1;
    }
    gpsfe_close(fe);
    if (*bad)
        return rc;
    /* one echo of the first channel's satellite, ten blocks */
    if (gpsfe_open(cfg, &fe) != GPSFE_OK) {
        snprintf(why, sizeof why, "a third gpsfe_open of the same file failed");
        *bad = 1;
        return rc;
    }
    int prn = 0;
    gpsfe_channel_info(fe, 0, &prn, NULL, NULL, NULL, NULL);
    const gpsfe_echo_t echo = {prn > 0 ? prn : 1, 150.0, 6.0, 0.25, 0.5};
    if (gpsfe_set_echoes(fe, &echo, 1) != GPSFE_OK || gpsfe_block_chans(fe) != MAX_CHAN + 1) {
        snprintf(why, sizeof why, "gpsfe_set_echoes refused one echo");
        *bad = 1;
    }
    for (int b = 0; b < 10 && !*bad; b++)
        if (gpsfe_next_block(fe, blk) != GPSFE_OK || !desc_ok(blk, MAX_CHAN + 1, "next_block with an echo"))
            *bad = 1;
    gpsfe_close(fe);
    return rc;
}

static void child(const char *path, const char *goodnav, int kind, long limit_ms, int out_fd)
{
    struct itimerval it;
    memset(&it, 0, sizeof it);
    it.it_value.tv_sec = limit_ms / 1000;
    it.it_value.tv_usec = (limit_ms % 1000) * 1000;
    signal(SIGALRM, SIG_DFL);
    setitimer(ITIMER_REAL, &it, NULL); /* SIGALRM ends the process, whatever thread spins */

    gpsfe_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.navfile = kind == 2 ? goodnav : path;
    cfg.rinex3 = kind == 1;
    cfg.motion_file = kind == 2 ? path : NULL;
    cfg.pos[0] = 30.286502, cfg.pos[1] = 120.032669, cfg.pos[2] = 100.0;
    cfg.max_chan = MAX_CHAN;

    int bad = 0;
    char sets[128] = "sets=- valid=-", line[640];
    const int rc = run_config(&cfg, &bad, sets, sizeof sets);
    int rct = 0;
    if (!bad) {
        cfg.have_start = 1, cfg.time_overwrite = 1;
        cfg.y = 2014, cfg.m = 12, cfg.d = 21, cfg.hh = 10, cfg.mm = 0, cfg.sec = 0.0;
        rct = run_config(&cfg, &bad, NULL, 0);
    }
    int rcr = 0;
    if (!bad) { /* from 20 s before the 01:00 set becomes current: the roll-over to the next set inside the run */
        cfg.time_overwrite = 0;
        cfg.d = 20, cfg.hh = 0, cfg.mm = 59, cfg.sec = 40.0;
        rcr = run_config(&cfg, &bad, NULL, 0);
    }
    const int n = snprintf(line, sizeof line, "open=%d %s openT=%d openR=%d end=%s%s\n", rc, sets, rct, rcr, bad ? "baddesc: " : "ok",
                           bad ? why : "");
    if (write(out_fd, line, (size_t)n) != n)
        _exit(4);
    exit(bad ? EXIT_BADDESC : 0);
}

static int by_name(const struct dirent **a, const struct dirent **b) { return strcmp((*a)->d_name, (*b)->d_name); }

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: %s CASEDIR GOODNAV LIMIT_MS\n", argv[0]);
        return 2;
    }
    const long limit_ms = atol(argv[3]);
    struct dirent **names = NULL;
    const int n = scandir(argv[1], &names, NULL, by_name);
    if (n < 0 || limit_ms < 1) {
        fprintf(stderr, "%s: cannot list %s, or no time limit\n", argv[0], argv[1]);
        return 2;
    }
    int failed = 0;
    for (int k = 0; k < n; k++) {
        const char *name = names[k]->d_name, *dot = strrchr(name, '.');
        const int kind = !dot ? -1 : !strcmp(dot, ".n2") ? 0 : !strcmp(dot, ".n3") ? 1 : !strcmp(dot, ".csv") ? 2 : -1;
        if (kind < 0)
            continue;
        char path[4096];
        snprintf(path, sizeof path, "%s/%s", argv[1], name);
        int fd[2];
        if (pipe(fd) != 0)
            return 2;
        fflush(stdout);
        fprintf(stderr, "== %s\n", name);
        fflush(stderr);
        const pid_t pid = fork();
        if (pid < 0)
            return 2;
        if (pid == 0) {
            close(fd[0]);
            child(path, argv[2], kind, limit_ms, fd[1]);
        }
        close(fd[1]);
        char line[640];
        size_t got = 0;
        ssize_t r;
        while (got < sizeof line - 1 && (r = read(fd[0], line + got, sizeof line - 1 - got)) > 0)
            got += (size_t)r;
        line[got] = 0;
        close(fd[0]);
        int st = 0;
        waitpid(pid, &st, 0);
        if (WIFSIGNALED(st)) {
            if (WTERMSIG(st) == SIGALRM)
                printf("%s end=timeout\n", name);
            else
                printf("%s end=signal %d\n", name, WTERMSIG(st));
            failed++;
        } else if (WEXITSTATUS(st) == 0 || WEXITSTATUS(st) == EXIT_BADDESC) {
            printf("%s %s", name, got ? line : "end=exit without a result\n");
            failed += WEXITSTATUS(st) != 0 || !got;
        } else {
            printf("%s end=exit %d\n", name, WEXITSTATUS(st));
            failed++;
        }
        free(names[k]);
    }
    free(names);
    return failed ? 1 : 0;
}
