// The host-side rules of the acquisition search (csrc/gpsbb_acq.h) under the host sanitizers, on a machine without a GPU: the bound
// and the smallest shift over the whole range of N and nnc, gpsbb_acq_make at the edges of every argument, the configuration check
// field by field, gpsbb_acq_best on rows whose sums carry into the high word.  Prints one line per group; exit status 1 on a
// finding.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipluto-gps-sim_amd/csrc tools/acq_asan.cpp -o acq_asan
//   ./acq_asan
// Never loaded into Python, never run on a GPU: nothing here makes a HIP call.
#include <stdio.h>

#include <vector>

#include "gpsbb_acq.h"

using namespace gpsbb_impl;

static int bad = 0;
#define EXPECT(c)                                              \
    do {                                                       \
        if (!(c)) {                                            \
            printf("acq_asan: %s (line %d)\n", #c, __LINE__); \
            bad++;                                             \
        }                                                      \
    } while (0)

int main()
{
    const unsigned views[3] = {GPSBB_OUT_SC16, GPSBB_OUT_SC8(5), GPSBB_OUT_SC1};
    int sh8 = 0;
    // the smallest shift is legal and the one below it is not, everywhere
    long n = 0;
    for (unsigned v : views)
        for (int nnc : {1, 2, 3, 63, 64})
            for (long ncoh = 1; ncoh <= ACQ_MAX_NCOH; ncoh = ncoh < 64 ? ncoh + 1 : ncoh * 2 - 7) {
                const int fmt = acq_view_format(v, &sh8);
                const int a = acq_min_shift(v, (int)ncoh, nnc);
                EXPECT(a >= 0 && a <= ACQ_MAX_SHIFT && acq_fits(fmt, (int)ncoh, nnc, a) && (a == 0 || !acq_fits(fmt, (int)ncoh, nnc, a - 1)));
                n++;
            }
    EXPECT(acq_min_shift(GPSBB_OUT_SC16, ACQ_MAX_NCOH, ACQ_MAX_NNC) <= ACQ_MAX_SHIFT);
    EXPECT(acq_min_shift(GPSBB_OUT_SC16, 2600, 2) == 6 && acq_min_shift(GPSBB_OUT_SC1, 2600, 2) == 0);
    EXPECT(acq_min_shift(3u << 8, 100, 1) == GPSBB_E_BADARG && acq_min_shift(0, 0, 1) == GPSBB_E_BADARG &&
           acq_min_shift(0, ACQ_MAX_NCOH + 1, 1) == GPSBB_E_BADARG && acq_min_shift(0, 1, 65) == GPSBB_E_BADARG);
    printf("min_shift: %ld points\n", n);

    // make: the three rates of the tests in every view, then the edges of every argument
    gpsbb_acq_cfg_t c;
    n = 0;
    for (double fs : {2.6e6, 3.0e6, 25e6})
        for (unsigned v : views) {
            EXPECT(acq_make(&c, 1.0 / fs, -5000.0, 500.0, 21, 1e-3, 0, 2, v) == GPSBB_OK);
            EXPECT(c.nbins == 21 && c.step[10] == 0 && c.step[0] < 0 && c.step[20] > 0 && c.nlags == (int)(fs / 1000.0 + 0.5) && c.ncoh == c.nlags);
            const long need = (long)c.nnc * c.ncoh + c.nlags - 1;
            EXPECT(acq_cfg_ok(&c, acq_view_format(v, &sh8), need) && !acq_cfg_ok(&c, acq_view_format(v, &sh8), need - 1));
            n++;
        }
    const double d = 1.0 / 2.6e6;
    EXPECT(acq_make(&c, d, -0.4999 / d, 0.9998 / d, 2, 1e-3, 1, 1, 0) == GPSBB_OK && c.step[0] < 0 && c.step[1] > 0);
    EXPECT(acq_make(&c, 0x1p-21, -0x1p+20, 0.0, 1, 1e-3, 1, 1, 0) == GPSBB_E_BADARG); /* |f delt| = 0.5 exactly */
    EXPECT(acq_make(&c, d, 0.0, 0.0, GPSBB_ACQ_MAX_BINS, 1e-3, ACQ_MAX_LAGS, ACQ_MAX_NNC, GPSBB_OUT_SC8(15)) == GPSBB_OK);
    EXPECT(acq_make(&c, d, 0.0, 0.0, GPSBB_ACQ_MAX_BINS + 1, 1e-3, 1, 1, 0) == GPSBB_E_BADARG);
    EXPECT(acq_make(&c, d, 0.0, 0.0, 1, 1e-3, ACQ_MAX_LAGS + 1, 1, 0) == GPSBB_E_BADARG);
    EXPECT(acq_make(&c, d, 0.0, 0.0, 1, 1e300, 1, 1, 0) == GPSBB_E_BADARG && acq_make(&c, d, 0.0, 0.0, 1, 1e-300, 1, 1, 0) == GPSBB_E_BADARG);
    EXPECT(acq_make(&c, 1e-300, 0.0, 0.0, 1, 1e-3, 1, 1, 0) == GPSBB_E_BADARG && acq_make(&c, 1e300, 0.0, 0.0, 1, 1e-3, 1, 1, 0) == GPSBB_E_BADARG);
    EXPECT(acq_make(&c, 2e-6, 0.0, 0.0, 1, 1e-3, 1, 1, 0) == GPSBB_E_BADARG);           /* more than 1.5 chips per sample */
    EXPECT(acq_make(&c, 1e-8, 0.0, 0.0, 1, 1e-4, 0, 1, 0) == GPSBB_E_BADARG);           /* a code period of 100000 samples */
    EXPECT(acq_make(nullptr, d, 0.0, 0.0, 1, 1e-3, 1, 1, 0) == GPSBB_E_BADARG);
    printf("make: %ld configurations and the edges\n", n);

    // the configuration check, one field wrong at a time
    EXPECT(acq_make(&c, d, -5000.0, 500.0, 21, 1e-3, 0, 2, 0) == GPSBB_OK);
    const long need = (long)c.nnc * c.ncoh + c.nlags - 1;
    n = 0;
    auto refused = [&](gpsbb_acq_cfg_t x) {
        n++;
        return !acq_cfg_ok(&x, 0, need + (1l << 27));
    };
    gpsbb_acq_cfg_t x;
    x = c; x.prn_mask = 0; EXPECT(refused(x));
    x = c; x.nbins = 0; EXPECT(refused(x));
    x = c; x.nbins = GPSBB_ACQ_MAX_BINS + 1; EXPECT(refused(x));
    x = c; x.code_step = 0; EXPECT(refused(x));
    x = c; x.code_step = ACQ_MAX_CODE_STEP + 1; EXPECT(refused(x));
    x = c; x.code_step = ACQ_MAX_CODE_STEP; EXPECT(!refused(x));
    x = c; x.ncoh = 0; EXPECT(refused(x));
    x = c; x.ncoh = ACQ_MAX_NCOH + 1; x.shift = 31; EXPECT(refused(x));
    x = c; x.ncoh = ACQ_MAX_NCOH; x.nnc = ACQ_MAX_NNC; x.nlags = ACQ_MAX_LAGS; x.shift = 31; EXPECT(!refused(x));
    x = c; x.nlags = 0; EXPECT(refused(x));
    x = c; x.nlags = ACQ_MAX_LAGS + 1; EXPECT(refused(x));
    x = c; x.nnc = 0; EXPECT(refused(x));
    x = c; x.nnc = ACQ_MAX_NNC + 1; x.shift = 31; EXPECT(refused(x));
    x = c; x.shift = -1; EXPECT(refused(x));
    x = c; x.shift = 32; EXPECT(refused(x));
    x = c; x.shift = c.shift - 1; EXPECT(refused(x));
    EXPECT(!acq_cfg_ok(nullptr, 0, need) && !acq_cfg_ok(&c, -1, need) && acq_cfg_ok(&c, 0, need));
    printf("cfg_ok: %ld configurations\n", n);

    // best: ties to the lowest bin, 128-bit sums with carries, rows at the end of the array
    std::vector<gpsbb_acq_row_t> rows((size_t)ACQ_PRNS * c.nbins);
    memset(rows.data(), 0, rows.size() * sizeof rows[0]);
    gpsbb_acq_row_t *r = rows.data() + (size_t)31 * c.nbins;
    for (int k = 0; k < c.nbins; k++) {
        r[k].peak = k == 3 || k == 20 ? ~0ull : (uint64_t)k;
        r[k].lag = 100 + k;
        r[k].sum_lo = ~0ull;
        r[k].sum_hi = (uint64_t)k;
    }
    int bin = -1, lag = -1;
    uint64_t peak = 0;
    double ratio = 0.0;
    EXPECT(acq_best(rows.data(), &c, 32, &bin, &lag, &peak, &ratio) == GPSBB_OK && bin == 3 && lag == 103 && peak == ~0ull);
    const double sum = (210.0 + 21.0) * 0x1p+64 - 21.0;
    EXPECT(ratio > 0.0 && ratio == 0x1p+64 / (sum / (21.0 * c.nlags)));
    EXPECT(acq_best(rows.data(), &c, 1, &bin, &lag, &peak, &ratio) == GPSBB_OK && bin == 0 && lag == 0 && peak == 0 && ratio == 0.0);
    EXPECT(acq_best(rows.data(), &c, 32, nullptr, nullptr, nullptr, nullptr) == GPSBB_OK);
    EXPECT(acq_best(rows.data(), &c, 0, &bin, &lag, &peak, &ratio) == GPSBB_E_BADARG && acq_best(rows.data(), &c, 33, &bin, &lag, &peak, &ratio) == GPSBB_E_BADARG);
    EXPECT(acq_best(nullptr, &c, 1, &bin, &lag, &peak, &ratio) == GPSBB_E_BADARG && acq_best(rows.data(), nullptr, 1, &bin, &lag, &peak, &ratio) == GPSBB_E_BADARG);
    printf("best: done\nacq_asan: %d findings\n", bad);
    return bad ? 1 : 0;
}
