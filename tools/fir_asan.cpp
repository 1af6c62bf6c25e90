// The host-side rules of the front-end filter (csrc/gpsbb_fir.h) under the host sanitizers, on a machine without a GPU: the
// rounding and the clamp at the ends of the accumulator's range, the checks of a gpsbb_fir_t at the corners of every field,
// gpsbb_fir_make over a grid of arguments and at the edges of each, and fir_host, the definition in plain C, against a brute-force
// restatement in 64-bit integers: random data, the longest filter, histories present, absent and in place, buffers shorter than
// the history, a buffer split into calls.  Prints one line per finding; exit status 1 on a finding.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipluto-gps-sim_amd/csrc tools/fir_asan.cpp -o fir_asan
//   ./fir_asan
// Never loaded into Python, never run on a GPU: nothing here makes a HIP call.
#include <stdio.h>

#include <vector>

#include "gpsbb_fir.h"

using namespace gpsbb_impl;

static int bad = 0;
#define EXPECT(c)                                              \
    do {                                                       \
        if (!(c)) {                                            \
            printf("fir_asan: %s (line %d)\n", #c, __LINE__); \
            bad++;                                             \
        }                                                      \
    } while (0)

static uint64_t rng_state = 0xf1ac0ffee54321ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

// taps with the sum of |h| exactly `budget`, signs random
static gpsbb_fir_t random_fir(int T, int D, int shift, int budget)
{
    gpsbb_fir_t f;
    memset(&f, 0, sizeof f);
    f.ntaps = T;
    f.decim = D;
    f.shift = shift;
    int left = budget;
    for (int k = 0; k < T; k++) {
        const int most = left < 32767 ? left : 32767;
        const int v = k == T - 1 ? most : (int)rnd_in(0, most);
        f.h[k] = (int16_t)(rnd() & 1 ? -v : v);
        left -= v;
    }
    return f;
}

// the definition once more, in 64-bit integers over one concatenated array
static void brute(const gpsbb_fir_t &f, const std::vector<int16_t> &hist, const std::vector<int16_t> &w, std::vector<int16_t> &y,
                  std::vector<int16_t> &tail, uint64_t &clips)
{
    const int T = f.ntaps, D = f.decim;
    std::vector<int16_t> x(hist);
    x.insert(x.end(), w.begin(), w.end());
    const long nsamp = (long)w.size() / 2;
    y.assign((size_t)(nsamp / D) * 2, 0);
    clips = 0;
    for (long m = 0; m < nsamp / D; m++)
        for (int c = 0; c < 2; c++) {
            int64_t acc = 0;
            for (int k = 0; k < T; k++)
                acc += (int64_t)f.h[k] * (int64_t)x[(size_t)(2 * (T - 1 + m * D + D - 1 - k) + c)];
            int64_t r = acc;
            if (f.shift)
                r = (acc + ((int64_t)1 << (f.shift - 1))) >> f.shift;
            const int64_t v = r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
            clips += v != r;
            y[(size_t)(2 * m + c)] = (int16_t)v;
        }
    tail.assign(x.end() - 2 * (T - 1), x.end());
}

static std::vector<int16_t> random_iq(long n)
{
    std::vector<int16_t> v((size_t)n * 2);
    for (auto &e : v)
        e = (int16_t)rnd_in(-32768, 32767);
    if (n >= 2) {
        v[0] = 32767;
        v[1] = -32768;
        v[2] = -32768;
        v[3] = 32767;
    }
    return v;
}

static void check_host(const gpsbb_fir_t &f, long nsamp, bool with_hist)
{
    const int T = f.ntaps;
    std::vector<int16_t> hist = with_hist ? random_iq(T - 1) : std::vector<int16_t>((size_t)(T - 1) * 2, 0);
    const std::vector<int16_t> w = random_iq(nsamp);
    std::vector<int16_t> want, want_tail, got((size_t)(nsamp / f.decim) * 2), tail((size_t)(T - 1) * 2 + 2, 0x55);
    uint64_t want_clips = 0, clips = ~0ull;
    brute(f, hist, w, want, want_tail, want_clips);
    EXPECT(fir_host(&f, w.data(), nsamp, with_hist ? hist.data() : nullptr, tail.data(), got.data(), &clips));
    EXPECT(got == want && clips == want_clips);
    EXPECT(std::vector<int16_t>(tail.begin(), tail.end() - 2) == want_tail && tail[tail.size() - 1] == 0x55 && tail[tail.size() - 2] == 0x55);
    if (with_hist && T > 1) { // the history in place, no clip count
        std::vector<int16_t> inplace(hist), again(got.size());
        EXPECT(fir_host(&f, w.data(), nsamp, inplace.data(), inplace.data(), again.data(), nullptr));
        EXPECT(again == want && inplace == want_tail);
    }
}

int main()
{
    // rounding and clamp: the ends of the accumulator's range at the largest shift, halves toward +infinity
    const int32_t top = 65535 * 32768, low = -65535 * 32768;
    EXPECT(fir_round(top, 16) == 32768 && fir_round(low, 16) == -32767 && fir_round(top, 0) == top && fir_round(low, 0) == low);
    EXPECT(fir_round(1, 1) == 1 && fir_round(-1, 1) == 0 && fir_round(-3, 1) == -1 && fir_round(3, 1) == 2 && fir_round(-2, 1) == -1);
    EXPECT(fir_round(32767, 16) == 0 && fir_round(32768, 16) == 1 && fir_round(-32768, 16) == 0 && fir_round(-32769, 16) == -1);
    for (int i = 0; i < 20000; i++) {
        const int32_t acc = (int32_t)rnd_in(low, top);
        const int s = (int)rnd_in(1, 16);
        EXPECT((int64_t)fir_round(acc, s) == (((int64_t)acc + ((int64_t)1 << (s - 1))) >> s));
    }
    EXPECT(fir_clamp(32768) == 32767 && fir_clamp(-32769) == -32768 && fir_clamp(32767) == 32767 && fir_clamp(-32768) == -32768);

    // fir_ok: every field at both ends of its range and one beyond
    gpsbb_fir_t f = random_fir(33, 4, 15, 40000);
    EXPECT(fir_ok(&f) && !fir_ok(nullptr));
    for (int T : {0, -1, GPSBB_FIR_MAX_TAPS + 1}) { gpsbb_fir_t g = f; g.ntaps = T; EXPECT(!fir_ok(&g)); }
    for (int D : {0, -1, 17}) { gpsbb_fir_t g = f; g.decim = D; EXPECT(!fir_ok(&g)); }
    for (int s : {-1, 17}) { gpsbb_fir_t g = f; g.shift = s; EXPECT(!fir_ok(&g)); }
    for (int s : {0, 16}) { gpsbb_fir_t g = f; g.shift = s; EXPECT(fir_ok(&g)); }
    { gpsbb_fir_t g = random_fir(GPSBB_FIR_MAX_TAPS, 16, 16, 65535); EXPECT(fir_ok(&g)); g.h[0] = (int16_t)(g.h[0] < 0 ? g.h[0] - 1 : g.h[0] + 1); EXPECT(!fir_ok(&g)); }
    { gpsbb_fir_t g = random_fir(1, 1, 0, 0); g.h[0] = -32768; EXPECT(fir_ok(&g)); }
    { gpsbb_fir_t g = random_fir(3, 1, 0, 0); g.h[0] = -32768; g.h[1] = 32767; g.h[2] = 1; EXPECT(!fir_ok(&g)); g.h[2] = 0; EXPECT(fir_ok(&g)); }
    { gpsbb_fir_t g; memset(&g, 0, sizeof g); g.ntaps = GPSBB_FIR_MAX_TAPS; g.decim = 1; for (auto &v : g.h) v = -32768; EXPECT(!fir_ok(&g)); }

    // fir_make: a grid, and the edges of every argument
    int made = 0;
    for (int T = 1; T <= GPSBB_FIR_MAX_TAPS; T += (T < 12 ? 1 : 7))
        for (int D = 1; D <= 16; D++)
            for (double cutoff : {0.0, 0.05, 0.5, 0.8, 1.0})
                for (double a : {0.0, 10.0, 21.0, 50.0, 60.0, 100.0, 180.0}) {
                    gpsbb_fir_t g;
                    memset(&g, 0x5a, sizeof g);
                    const int rc = fir_make(&g, T, D, cutoff, a);
                    if (rc != GPSBB_OK) { // only a result whose taps do not fit may be refused here
                        EXPECT(rc == GPSBB_E_BADARG && g.ntaps == 0x5a5a5a5a);
                        continue;
                    }
                    made++;
                    int32_t sum = 0;
                    bool sym = true;
                    for (int k = 0; k < T; k++) {
                        sum += g.h[k];
                        sym = sym && (g.h[k] == g.h[T - 1 - k] || (T % 2 == 0 && (k == T / 2 - 1 || k == T / 2))); // (an even T's residual)
                    }
                    EXPECT(fir_ok(&g) && g.ntaps == T && g.decim == D && (g.shift == 15 || g.shift == 14) && sum == 1 << g.shift && sym);
                }
    EXPECT(made > 5000);
    gpsbb_fir_t one;
    EXPECT(fir_make(&one, 1, 1, 0.0, 0.0) == GPSBB_OK && one.shift == 14 && one.h[0] == 16384);
    EXPECT(fir_make(nullptr, 33, 4, 0.8, 60.0) == GPSBB_E_BADARG && fir_make(&one, 0, 4, 0.8, 60.0) == GPSBB_E_BADARG);
    EXPECT(fir_make(&one, GPSBB_FIR_MAX_TAPS + 1, 4, 0.8, 60.0) == GPSBB_E_BADARG && fir_make(&one, 33, 0, 0.8, 60.0) == GPSBB_E_BADARG);
    EXPECT(fir_make(&one, 33, 17, 0.8, 60.0) == GPSBB_E_BADARG && fir_make(&one, 33, 4, 1.0000001, 60.0) == GPSBB_E_BADARG);
    EXPECT(fir_make(&one, 33, 4, NAN, 60.0) == GPSBB_E_BADARG && fir_make(&one, 33, 4, 0.8, INFINITY) == GPSBB_E_BADARG);
    EXPECT(fir_make(&one, 33, 4, -INFINITY, 60.0) == GPSBB_E_BADARG && fir_make(&one, 33, 4, 0.8, 180.5) == GPSBB_E_BADARG);
    EXPECT(one.shift == 14 && one.h[0] == 16384); // a refusal writes nothing
    EXPECT(fir_make(&one, GPSBB_FIR_MAX_TAPS, 16, 1.0, 180.0) == GPSBB_OK && fir_make(&one, 33, 4, -1.0, -1.0) == GPSBB_OK);
    gpsbb_fir_t dflt;
    EXPECT(fir_make(&dflt, 33, 4, 0.8, 60.0) == GPSBB_OK && !memcmp(&dflt, &one, sizeof one));
    EXPECT(fir_i0(0.0) == 1.0 && fabs(fir_i0(1.0) - 1.2660658777520084) < 1e-15 && fabs(fir_i0(2.0) - 2.2795853023360673) < 1e-14);

    // fir_host against brute force
    for (int T : {1, 2, 5, 33, 64, 128, GPSBB_FIR_MAX_TAPS})
        for (int D : {1, 3, 4, 7, 16})
            for (int shift : {0, 1, 15, 16}) {
                const gpsbb_fir_t g = random_fir(T, D, shift, shift ? 65535 : (int)rnd_in(0, 3));
                check_host(g, (long)D * rnd_in(1, 40), true);
                check_host(g, (long)D, false); // one output; for T - 1 > D part of the history survives
            }
    // every component -32768 under the largest taps: the accumulator at the end of its range, every component clipped at shift 0
    {
        gpsbb_fir_t g = random_fir(3, 1, 0, 0);
        g.h[0] = g.h[1] = 32767;
        g.h[2] = 1;
        std::vector<int16_t> w(64, -32768), hist(4, -32768), y(64), tail(4);
        uint64_t clips = 0;
        EXPECT(fir_host(&g, w.data(), 32, hist.data(), tail.data(), y.data(), &clips) && clips == 64 && y[0] == -32768 && y[63] == -32768);
        g.shift = 16;
        EXPECT(fir_host(&g, w.data(), 32, hist.data(), tail.data(), y.data(), &clips) && clips == 0 && y[0] == -32767 && y[63] == -32767);
    }
    // one call == a split at multiples of D, a piece shorter than T - 1 among them
    {
        const gpsbb_fir_t g = random_fir(33, 4, 15, 65535);
        const std::vector<int16_t> w = random_iq(400);
        std::vector<int16_t> whole(200), parts(200), t0(64, 0), t1(64, 0);
        uint64_t c0 = 0, c1 = 0, c = 0;
        EXPECT(fir_host(&g, w.data(), 400, nullptr, t0.data(), whole.data(), &c0));
        long at = 0;
        for (long n : {4L, 200L, 8L, 188L}) {
            EXPECT(fir_host(&g, w.data() + 2 * at, n, t1.data(), t1.data(), parts.data() + 2 * (at / 4), &c));
            c1 += c;
            at += n;
        }
        EXPECT(at == 400 && parts == whole && t0 == t1 && c0 == c1);
    }
    // refusals of fir_host
    {
        const gpsbb_fir_t g = random_fir(5, 3, 1, 100);
        std::vector<int16_t> w(12), y(4);
        EXPECT(!fir_host(&g, w.data(), 0, nullptr, nullptr, y.data(), nullptr) && !fir_host(&g, w.data(), 4, nullptr, nullptr, y.data(), nullptr));
        EXPECT(!fir_host(&g, nullptr, 3, nullptr, nullptr, y.data(), nullptr) && !fir_host(&g, w.data(), 3, nullptr, nullptr, nullptr, nullptr));
        EXPECT(fir_host(&g, w.data(), 6, nullptr, nullptr, y.data(), nullptr));
    }
    if (bad)
        return 1;
    printf("fir_asan: rounding, checks, %d designs, fir_host against brute force: clean\n", made);
    return 0;
}
