// The host-side rules of the tracking loops (csrc/gpsbb_track.h) under the host sanitizers, on a machine without a GPU: closing an
// epoch (steps 4-8, the arithmetic k_track's closing lane runs) over operands at the ends of every range, an epoch's geometry
// (steps 1-2), the configuration and state checks field by field, gpsbb_trk_make at the edges of every argument, the seed, bit
// edge and bits on records at the end of their array.  Prints one line per group; exit status 1 on a finding.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipluto-gps-sim_amd/csrc tools/track_asan.cpp -o track_asan
//   ./track_asan
// Never loaded into Python, never run on a GPU: nothing here makes a HIP call.
#include <stdio.h>

#include <vector>

#include "gpsbb_acq.h"
#include "gpsbb_track.h"

using namespace gpsbb_impl;

static int bad = 0;
#define EXPECT(c)                                                \
    do {                                                         \
        if (!(c)) {                                              \
            printf("track_asan: %s (line %d)\n", #c, __LINE__); \
            bad++;                                               \
        }                                                        \
    } while (0)

static uint64_t rng_state = 0x7ac0ffee12345ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

static gpsbb_trk_cfg_t good_cfg()
{
    gpsbb_trk_cfg_t c;
    EXPECT(trk_make(&c, 1.0 / 2.6e6, 0.0, 0.0, 0.0, 0, 0) == GPSBB_OK);
    return c;
}

int main()
{
    // m(x)
    EXPECT(trk_m(0) == 0 && trk_m(-1) == 0 && trk_m(1) == 1 && trk_m(-2) == 1 && trk_m((1 << 20) - 1) == 20 && trk_m(1 << 20) == 21 &&
           trk_m(-(1 << 20)) == 20 && trk_m(-(1 << 20) - 1) == 21 && trk_m(INT64_MAX) == 63 && trk_m(INT64_MIN) == 63);

    // make: the rates of the tests, then the edges of every argument
    gpsbb_trk_cfg_t c = good_cfg();
    EXPECT(c.code_nom == 1689904440ull && c.aid_div == (1540ll << 16) && c.spacing == (1u << 31) && c.nfll == 100 && c.max_epochs == 1000);
    EXPECT(c.kf == 157746 && c.kp1 == 42085 && c.kp2 == 842 && c.kd1 == 645 && c.kd2 == 0 && trk_cfg_ok(&c));
    gpsbb_trk_cfg_t c25;
    EXPECT(trk_make(&c25, 1.0 / 25e6, 0.3, 30.0, 0.2, 7, TRK_MAX_EPOCHS) == GPSBB_OK && c25.nfll == 7 && c25.max_epochs == TRK_MAX_EPOCHS && trk_cfg_ok(&c25));
    EXPECT(trk_make(nullptr, 1e-6, 0, 0, 0, 0, 0) == GPSBB_E_BADARG && trk_make(&c25, 0.0, 0, 0, 0, 0, 0) == GPSBB_E_BADARG);
    EXPECT(trk_make(&c25, NAN, 0, 0, 0, 0, 0) == GPSBB_E_BADARG && trk_make(&c25, INFINITY, 0, 0, 0, 0, 0) == GPSBB_E_BADARG);
    EXPECT(trk_make(&c25, 1e-6, NAN, 0, 0, 0, 0) == GPSBB_E_BADARG && trk_make(&c25, 1e-6, 0, INFINITY, 0, 0, 0) == GPSBB_E_BADARG);
    EXPECT(trk_make(&c25, 1e-6, 0, 0, NAN, 0, 0) == GPSBB_E_BADARG && trk_make(&c25, 1e-6, 0, 0, 0, 0, TRK_MAX_EPOCHS + 1) == GPSBB_E_BADARG);
    EXPECT(trk_make(&c25, 2e-6, 0, 0, 0, 0, 0) == GPSBB_E_BADARG);   /* more than 1.5 chips per sample */
    EXPECT(trk_make(&c25, 1e-10, 0, 0, 0, 0, 0) == GPSBB_E_BADARG);  /* a code period beyond 2^20 samples */
    EXPECT(trk_make(&c25, 1e-6, 1e300, 0, 0, 0, 0) == GPSBB_E_BADARG && trk_make(&c25, 1e-6, 0, 1e200, 0, 0, 0) == GPSBB_E_BADARG &&
           trk_make(&c25, 1e-6, 0, 0, 1e300, 0, 0) == GPSBB_E_BADARG); /* gains beyond int32 */
    printf("make: done\n");

    // the configuration check, one field wrong at a time, and the smallest code_nom
    uint64_t nom_min = (TRK_LEN >> 20) * 8 / 7;
    while ((TRK_LEN + (nom_min - nom_min / 8) - 1) / (nom_min - nom_min / 8) > (uint64_t)TRK_MAX_N)
        nom_min++;
    gpsbb_trk_cfg_t x;
    x = c; x.code_nom = 0; EXPECT(!trk_cfg_ok(&x));
    x = c; x.code_nom = TRK_MAX_CODE_NOM + 1; EXPECT(!trk_cfg_ok(&x));
    x = c; x.code_nom = TRK_MAX_CODE_NOM; EXPECT(trk_cfg_ok(&x));
    x = c; x.code_nom = nom_min; EXPECT(trk_cfg_ok(&x));
    x = c; x.code_nom = nom_min - 1; EXPECT(!trk_cfg_ok(&x));
    x = c; x.code_nom = 1; EXPECT(!trk_cfg_ok(&x));
    x = c; x.spacing = 0; EXPECT(!trk_cfg_ok(&x));
    x = c; x.spacing = 0xffffffffu; EXPECT(trk_cfg_ok(&x));
    x = c; x.nfll = -1; EXPECT(!trk_cfg_ok(&x));
    x = c; x.max_epochs = 0; EXPECT(!trk_cfg_ok(&x));
    x = c; x.max_epochs = TRK_MAX_EPOCHS + 1; EXPECT(!trk_cfg_ok(&x));
    x = c; x.aid_div = INT64_MIN; x.kf = x.kp1 = x.kp2 = x.kd1 = x.kd2 = INT32_MIN; EXPECT(trk_cfg_ok(&x));
    EXPECT(!trk_cfg_ok(nullptr));
    printf("cfg_ok: done (smallest code_nom %llu)\n", (unsigned long long)nom_min);

    // the state check
    gpsbb_trk_state_t s0;
    memset(&s0, 0, sizeof s0);
    s0.prn = 1;
    const long nsamp = 5000;
    gpsbb_trk_state_t s;
    EXPECT(trk_state_ok(&s0, nsamp));
    s = s0; s.prn = 0; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.prn = 33; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.epoch = -1; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.epoch = TRK_MAX_EPOCH0 + 1; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.n0 = -1; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.n0 = nsamp + 1; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.n0 = nsamp; EXPECT(trk_state_ok(&s, nsamp));
    s = s0; s.code_phase = TRK_LEN; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.code_phase = TRK_LEN - 1; EXPECT(trk_state_ok(&s, nsamp));
    for (int64_t v : {(int64_t)1 << 47, -((int64_t)1 << 47), INT64_MAX, INT64_MIN}) {
        s = s0; s.carr_int = v; EXPECT(!trk_state_ok(&s, nsamp));
        s = s0; s.carr_step = v; EXPECT(!trk_state_ok(&s, nsamp));
        s = s0; s.code_int = v == ((int64_t)1 << 47) || v == -((int64_t)1 << 47) ? v * 1024 : v; EXPECT(!trk_state_ok(&s, nsamp));
        s = s0; s.code_adj = v == ((int64_t)1 << 47) || v == -((int64_t)1 << 47) ? v * 8 : v; EXPECT(!trk_state_ok(&s, nsamp));
    }
    s = s0; s.carr_int = TRK_CARR_MAX; s.carr_step = -TRK_CARR_MAX; s.code_int = -TRK_CODE_INT_MAX; s.code_adj = TRK_CODE_ADJ_MAX; EXPECT(trk_state_ok(&s, nsamp));
    s = s0; s.prev_i = INT64_MIN; s.prev_q = INT64_MAX; EXPECT(trk_state_ok(&s, nsamp)); /* epoch 0: not read */
    s = s0; s.epoch = 1; s.prev_i = 1 << 20; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.epoch = 1; s.prev_q = -(1 << 20) - 1; EXPECT(!trk_state_ok(&s, nsamp));
    s = s0; s.epoch = 1; s.prev_i = (1 << 20) - 1; s.prev_q = -(1 << 20); EXPECT(trk_state_ok(&s, nsamp));
    printf("state_ok: done\n");

    // plan and close: every legal corner at once, then random legal operands; UBSan watches every product, shift and division
    long n = 0;
    const int32_t gains[] = {INT32_MIN, INT32_MAX, 0, 1, -1, 157746};
    const int64_t sums_edge[] = {0, -1, 1, (1 << 20) - 1, 1 << 20, -(1 << 20), -(1 << 20) - 1, (int64_t)1 << 45, -((int64_t)1 << 45)};
    for (int round = 0; round < 200000; round++) {
        gpsbb_trk_cfg_t k = c;
        k.code_nom = round % 3 == 0 ? nom_min : (round % 3 == 1 ? TRK_MAX_CODE_NOM : (uint64_t)rnd_in((int64_t)nom_min, (int64_t)TRK_MAX_CODE_NOM));
        const int64_t divs[] = {0, 1, -1, 1540ll << 16, INT64_MIN, INT64_MAX};
        k.aid_div = divs[rnd() % 6];
        k.nfll = (int)(rnd() % 3) * 5;
        k.kf = gains[rnd() % 6]; k.kp1 = gains[rnd() % 6]; k.kp2 = gains[rnd() % 6]; k.kd1 = gains[rnd() % 6]; k.kd2 = gains[rnd() % 6];
        gpsbb_trk_state_t st = s0;
        st.prn = 1 + (int)(rnd() % 32);
        st.epoch = (int)(rnd() % 4) == 0 ? 0 : (int)(rnd() % 12);
        st.n0 = rnd_in(0, (int64_t)1 << 40);
        st.carr_phase = (uint32_t)rnd();
        st.carr_int = rnd() % 4 == 0 ? (rnd() & 1 ? TRK_CARR_MAX : -TRK_CARR_MAX) : rnd_in(-TRK_CARR_MAX, TRK_CARR_MAX);
        st.carr_step = rnd() % 4 == 0 ? (rnd() & 1 ? TRK_CARR_MAX : -TRK_CARR_MAX) : rnd_in(-TRK_CARR_MAX, TRK_CARR_MAX);
        st.code_phase = rnd() % 8 == 0 ? TRK_LEN - 1 : (rnd() % 8 == 0 ? 0 : rnd() % TRK_LEN);
        st.code_int = rnd() % 4 == 0 ? (rnd() & 1 ? TRK_CODE_INT_MAX : -TRK_CODE_INT_MAX) : rnd_in(-TRK_CODE_INT_MAX, TRK_CODE_INT_MAX);
        st.code_adj = rnd() % 4 == 0 ? (rnd() & 1 ? TRK_CODE_ADJ_MAX : -TRK_CODE_ADJ_MAX) : rnd_in(-TRK_CODE_ADJ_MAX, TRK_CODE_ADJ_MAX);
        st.prev_i = rnd() % 4 == 0 ? -(1 << 20) : rnd_in(-(1 << 20), (1 << 20) - 1);
        st.prev_q = rnd() % 4 == 0 ? (1 << 20) - 1 : rnd_in(-(1 << 20), (1 << 20) - 1);
        EXPECT(trk_cfg_ok(&k) && trk_state_ok(&st, (long)1 << 41));
        uint64_t cs;
        int64_t N;
        trk_plan(k, st, &cs, &N);
        const uint64_t lo = k.code_nom - k.code_nom / 8, hi = k.code_nom + k.code_nom / 8;
        EXPECT(cs >= lo && cs <= hi && N >= 1 && N <= TRK_MAX_N && st.code_phase + cs * (uint64_t)N >= TRK_LEN &&
               st.code_phase + cs * (uint64_t)(N - 1) < TRK_LEN);
        int64_t sum[6];
        const int width = (int)(rnd() % 46);
        for (int q = 0; q < 6; q++)
            sum[q] = rnd() % 5 == 0 ? sums_edge[rnd() % 9] : rnd_in(-((int64_t)1 << width), (int64_t)1 << width);
        gpsbb_trk_epoch_t rec;
        const gpsbb_trk_state_t before = st;
        trk_close(k, st, cs, N, sum, &rec);
        EXPECT(trk_state_ok(&st, (long)1 << 42) && st.epoch == before.epoch + 1 && st.n0 == before.n0 + N && rec.N == N && rec.n0 == before.n0);
        EXPECT(rec.e_c >= -16384 && rec.e_c <= 16384 && rec.e_d >= -16384 && rec.e_d <= 16384 && rec.q >= 0 && rec.q <= 26);
        EXPECT(rec.mode == (before.epoch < k.nfll ? 0 : 1) && rec.carr_step == before.carr_step && rec.code_phase == before.code_phase);
        n++;
    }
    printf("plan and close: %ld epochs\n", n);

    // a short run of epochs: a state closed again and again stays legal, whatever the gains
    {
        gpsbb_trk_cfg_t k = c;
        k.kf = k.kp1 = k.kd1 = INT32_MAX;
        k.kp2 = k.kd2 = INT32_MIN;
        k.nfll = 50;
        gpsbb_trk_state_t st = s0;
        for (int e = 0; e < 100; e++) {
            uint64_t cs;
            int64_t N;
            trk_plan(k, st, &cs, &N);
            int64_t sum[6];
            for (int q = 0; q < 6; q++)
                sum[q] = rnd_in(-((int64_t)1 << 45), (int64_t)1 << 45);
            gpsbb_trk_epoch_t rec;
            trk_close(k, st, cs, N, sum, &rec);
            EXPECT(trk_state_ok(&st, (long)1 << 40));
        }
        printf("100 epochs at the largest gains: epoch %d, n0 %lld\n", st.epoch, (long long)st.n0);
    }

    // seed
    gpsbb_acq_cfg_t acq;
    EXPECT(acq_make(&acq, 1.0 / 2.6e6, -5000.0, 250.0, 41, 1e-3, 0, 2, 0) == GPSBB_OK);
    EXPECT(trk_seed(&s, &acq, 32, 40, 2599) == GPSBB_OK && s.prn == 32 && s.n0 == 2599 && s.carr_step == (int64_t)acq.step[40] * 65536 &&
           s.carr_int == s.carr_step && s.epoch == 0 && s.code_phase == 0 && trk_state_ok(&s, 2600));
    EXPECT(trk_seed(&s, &acq, 1, 0, 0) == GPSBB_OK && s.carr_step < 0);
    acq.step[0] = INT32_MIN;
    EXPECT(trk_seed(&s, &acq, 1, 0, 0) == GPSBB_OK && s.carr_step == -TRK_CARR_MAX && trk_state_ok(&s, 1));
    EXPECT(trk_seed(nullptr, &acq, 1, 0, 0) == GPSBB_E_BADARG && trk_seed(&s, nullptr, 1, 0, 0) == GPSBB_E_BADARG &&
           trk_seed(&s, &acq, 0, 0, 0) == GPSBB_E_BADARG && trk_seed(&s, &acq, 33, 0, 0) == GPSBB_E_BADARG &&
           trk_seed(&s, &acq, 1, -1, 0) == GPSBB_E_BADARG && trk_seed(&s, &acq, 1, 41, 0) == GPSBB_E_BADARG &&
           trk_seed(&s, &acq, 1, 0, -1) == GPSBB_E_BADARG);
    printf("seed: done\n");

    // bit edge and bits: the records end where their array ends, so a read beyond n is seen
    for (int len : {0, 1, 19, 20, 21, 47, 80}) {
        std::vector<gpsbb_trk_epoch_t> r((size_t)len);
        for (int k = 0; k < len; k++) {
            memset(&r[(size_t)k], 0, sizeof r[0]);
            r[(size_t)k].p_i = (((k + 13) / 20) & 1 ? -1 : 1) * (((int64_t)1 << 45) - k);
        }
        const gpsbb_trk_epoch_t *p = len ? r.data() : reinterpret_cast<const gpsbb_trk_epoch_t *>(&s0);
        int off = -1;
        int32_t hist[20];
        for (int skip : {0, 1, len - 1 > 0 ? len - 1 : 0, len, len + 5}) {
            EXPECT(trk_bitsync(p, len, skip, &off, hist) == GPSBB_OK && off >= 0 && off < 20);
            if (len >= 47 && skip == 0)
                EXPECT(off == 7 && hist[7] == (len - 7 + 19) / 20);
        }
        int8_t bits[8];
        for (int first : {0, 7, len, len + 1}) {
            const int nb = trk_bits(p, len, first, bits, 8);
            EXPECT(nb == (len - first >= 20 ? (len - first) / 20 : 0));
            EXPECT(trk_bits(p, len, first, bits, 1) == (nb > 0 ? 1 : 0) && trk_bits(p, len, first, bits, 0) == 0);
            if (first == 7 && nb > 0)
                EXPECT(bits[0] == -1);
        }
        EXPECT(trk_bitsync(p, len, 0, nullptr, nullptr) == GPSBB_OK);
        EXPECT(trk_bitsync(nullptr, len, 0, &off, hist) == GPSBB_E_BADARG && trk_bitsync(p, -1, 0, &off, hist) == GPSBB_E_BADARG &&
               trk_bitsync(p, len, -1, &off, hist) == GPSBB_E_BADARG);
        EXPECT(trk_bits(nullptr, len, 0, bits, 8) == GPSBB_E_BADARG && trk_bits(p, len, 0, nullptr, 8) == GPSBB_E_BADARG &&
               trk_bits(p, -1, 0, bits, 8) == GPSBB_E_BADARG && trk_bits(p, len, -1, bits, 8) == GPSBB_E_BADARG &&
               trk_bits(p, len, 0, bits, -1) == GPSBB_E_BADARG);
    }
    printf("bitsync and bits: done\ntrack_asan: %d findings\n", bad);
    return bad ? 1 : 0;
}
