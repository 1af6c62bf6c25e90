// The host-side rules of the power spectrum (csrc/gpsbb_psd.h) under the host sanitizers, on a machine without a GPU: the twiddle
// table's identities, the overflow bound on both sides of every shift, the checks of a gpsbb_psd_t at the corners of every field,
// gpsbb_psd_make's defaults, windows and refusals, and psd_host, the definition in plain C: every intermediate of the worst-case
// inputs inside int32 (the sanitizer sees a signed overflow), the transform against a DFT in doubles, the closed form of the
// constant input, one call against its split.  Prints one line per finding; exit status 1 on a finding.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipluto-gps-sim_amd/csrc tools/psd_asan.cpp -o psd_asan
//   ./psd_asan
// Never loaded into Python, never run on a GPU: nothing here makes a HIP call.
#include <stdio.h>

#include <vector>

#include "gpsbb_psd.h"

using namespace gpsbb_impl;

static int bad = 0;
#define EXPECT(c)                                              \
    do {                                                       \
        if (!(c)) {                                            \
            printf("psd_asan: %s (line %d)\n", #c, __LINE__); \
            bad++;                                             \
        }                                                      \
    } while (0)

static uint64_t rng_state = 0x95d0c0ffee1234ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

static int32_t tc[PSD_TW], ts[PSD_TW];

static gpsbb_psd_t plan(int log2n, int hop, int shift, int16_t fill)
{
    gpsbb_psd_t p;
    memset(&p, 0, sizeof p);
    p.log2n = log2n;
    p.hop = hop;
    p.shift = shift;
    for (auto &v : p.win)
        v = fill;
    return p;
}

static bool run(const gpsbb_psd_t &p, const std::vector<int16_t> &w, int fmt, std::vector<uint64_t> &out, long *nseg)
{
    std::vector<psd_c> work((size_t)2 << p.log2n);
    out.assign((size_t)1 << p.log2n, 0x5555555555555555ull);
    return psd_host(&p, w.data(), (long)w.size() / 2, fmt, tc, ts, work.data(), out.data(), nseg);
}

int main()
{
    // the table: the identities by construction, every entry within 1 of libm's
    psd_twiddles(tc, ts);
    EXPECT(tc[0] == 1 << 30 && ts[0] == 0 && tc[1024] == 0 && ts[1024] == 1 << 30 && tc[512] == ts[512]);
    for (int k = 1; k < PSD_TW; k++) {
        EXPECT(tc[2048 - k] == -tc[k] && ts[2048 - k] == ts[k]);
        EXPECT(fabs((double)tc[k] - ldexp(cos(2.0 * M_PI * k / 4096.0), 30)) <= 1.0 && fabs((double)ts[k] - ldexp(sin(2.0 * M_PI * k / 4096.0), 30)) <= 1.0);
        if (k <= 1024)
            EXPECT(tc[k] == ts[1024 - k]);
    }
    for (uint32_t x = 0; x < 2048; x++)
        EXPECT(psd_brev11(psd_brev11(x)) == x && psd_brev11(x) < 2048);
    EXPECT(psd_brev11(1) == 1024 && psd_brev11(2) == 512 && psd_brev11(3) == 1536);

    // the exact twiddles: t = v and t = -i v, at the ends of the range too
    for (int i = 0; i < 1000; i++) {
        const psd_c v{(int32_t)rnd_in(-(1 << 30), 1 << 30), (int32_t)rnd_in(-(1 << 30), 1 << 30)};
        const psd_c a = psd_tmul(v, tc[0], ts[0]), b = psd_tmul(v, tc[1024], ts[1024]);
        EXPECT(a.re == v.re && a.im == v.im && b.re == v.im && b.im == -v.re);
    }

    // the overflow rule: seven segments at shift 0, eight at shift 1; both sides of every shift
    EXPECT(psd_fits(7, 0) && !psd_fits(8, 0) && psd_fits(8, 1) && psd_min_shift(7) == 0 && psd_min_shift(8) == 1 && psd_min_shift(1) == 0);
    EXPECT(psd_min_shift(0) == GPSBB_E_BADARG && psd_min_shift(-1) == GPSBB_E_BADARG && psd_min_shift(PSD_MAX_NSEG + 1) == GPSBB_E_BADARG);
    EXPECT(psd_min_shift(PSD_MAX_NSEG) >= 0 && psd_min_shift(PSD_MAX_NSEG) <= 10 && !psd_fits(1, -1) && !psd_fits(1, 31) && psd_fits(PSD_MAX_NSEG, 30));
    for (long n = 1; n <= PSD_MAX_NSEG; n = n * 3 + 1) {
        const int s = psd_min_shift(n);
        const unsigned __int128 t = (((unsigned __int128)1 << 30) >> s) + 1;
        EXPECT((unsigned __int128)n * 2 * t * t < ((unsigned __int128)1 << 64) && (s == 0 || !psd_fits(n, s - 1)));
    }

    // psd_ok and psd_nseg: every field at both ends of its range and one beyond
    {
        gpsbb_psd_t p = plan(6, 64, 0, 16384);
        long n = 0;
        EXPECT(psd_ok(&p, 64, &n) && n == 1 && !psd_ok(&p, 63, &n) && !psd_ok(nullptr, 64, &n) && psd_ok(&p, 127, &n) && n == 1 && psd_ok(&p, 128, &n) && n == 2);
        for (int L : {5, 13, -1}) { gpsbb_psd_t q = p; q.log2n = L; EXPECT(!psd_ok(&q, 1 << 20, nullptr)); }
        for (int h : {0, -1, (1 << 20) + 1}) { gpsbb_psd_t q = p; q.hop = h; EXPECT(!psd_ok(&q, 1 << 22, nullptr)); }
        for (int s : {-1, 31}) { gpsbb_psd_t q = p; q.shift = s; EXPECT(!psd_ok(&q, 64, nullptr)); }
        { gpsbb_psd_t q = p; q.hop = 1 << 20; q.log2n = 12; q.shift = 30; EXPECT(psd_ok(&q, 4096, &n) && n == 1); }
        { gpsbb_psd_t q = p; q.hop = 1; q.shift = 30; EXPECT(psd_ok(&q, 64 + PSD_MAX_NSEG - 1, &n) && n == PSD_MAX_NSEG && !psd_ok(&q, 64 + PSD_MAX_NSEG, &n)); }
        { gpsbb_psd_t q = p; EXPECT(psd_ok(&q, 64 * 7, nullptr) && !psd_ok(&q, 64 * 8, nullptr)); q.shift = 1; EXPECT(psd_ok(&q, 64 * 8, nullptr)); }
    }

    // psd_make: defaults, windows, refusals; psd_scale
    {
        gpsbb_psd_t p, keep;
        memset(&p, 0x5a, sizeof p);
        keep = p;
        EXPECT(psd_make(&p, 5, 0, 0, 1 << 20) == GPSBB_E_BADARG && psd_make(&p, 13, 0, 0, 1 << 20) == GPSBB_E_BADARG && psd_make(nullptr, 6, 0, 0, 64) == GPSBB_E_BADARG);
        EXPECT(psd_make(&p, 6, 0, 2, 64) == GPSBB_E_BADARG && psd_make(&p, 6, 0, -1, 64) == GPSBB_E_BADARG && psd_make(&p, 6, 0, 0, 63) == GPSBB_E_BADARG);
        EXPECT(psd_make(&p, 6, (1 << 20) + 1, 0, 64) == GPSBB_E_BADARG && psd_make(&p, 6, 1, 0, 64 + PSD_MAX_NSEG) == GPSBB_E_BADARG);
        EXPECT(!memcmp(&p, &keep, sizeof p)); // a refusal writes nothing
        for (int L = PSD_MIN_LOG2N; L <= PSD_MAX_LOG2N; L++) {
            const int N = 1 << L;
            EXPECT(psd_make(&p, L, 0, 0, 8L * N + 5) == GPSBB_OK && p.hop == N && p.shift == 1 && p.log2n == L);
            for (int n = 0; n < GPSBB_PSD_MAX_N; n++)
                EXPECT(p.win[n] == (n < N ? 16384 : 0));
            EXPECT(fabs(psd_scale(&p, 8, 0) - 4.0 * 4.0 / (8.0 * 16384.0 * 16384.0)) < 1e-24);
            EXPECT(psd_make(&p, L, 0, 1, 4L * N) == GPSBB_OK && p.hop == N / 2 && p.shift == 0 && p.win[0] == 0 && p.win[N / 2] == 16384);
            for (int n = 1; n < N; n++)
                EXPECT(p.win[n] == p.win[N - n] && p.win[n] >= 0);
            EXPECT(psd_make(&p, L, 1 << 20, 1, N) == GPSBB_OK && p.hop == 1 << 20 && psd_make(&p, L, 1, 0, N + PSD_MAX_NSEG - 1) == GPSBB_OK);
        }
        gpsbb_psd_t z = plan(6, 64, 0, 0);
        EXPECT(std::isnan(psd_scale(&z, 1, 0)) && std::isnan(psd_scale(nullptr, 1, 0)) && std::isnan(psd_scale(&p, 0, 0)) && std::isnan(psd_scale(&p, 1, 3)));
    }

    // the worst cases of the range: nothing leaves int32 (the sanitizer would say so), and the constant's closed form
    for (int L : {6, 8, 11, 12}) {
        const int N = 1 << L;
        const long nsamp = 7L * N;
        std::vector<int16_t> con((size_t)nsamp * 2, -32768), alt((size_t)nsamp * 2), tone((size_t)nsamp * 2), rnd16((size_t)nsamp * 2);
        for (long n = 0; n < nsamp; n++) {
            alt[2 * n] = n & 1 ? -32768 : 32767;
            alt[2 * n + 1] = n & 1 ? 32767 : -32768;
            tone[2 * n] = (int16_t)nearbyint(32767.0 * cos(2.0 * M_PI * 5.0 * (double)n / N));
            tone[2 * n + 1] = (int16_t)nearbyint(32767.0 * sin(2.0 * M_PI * 5.0 * (double)n / N));
            rnd16[2 * n] = (int16_t)rnd_in(-32768, 32767);
            rnd16[2 * n + 1] = (int16_t)rnd_in(-32768, 32767);
        }
        const gpsbb_psd_t p = plan(L, N, 0, -32768);
        std::vector<uint64_t> out;
        long nseg = 0;
        EXPECT(run(p, con, 0, out, &nseg) && nseg == 7 && out[0] == 7ull * 2ull * (1ull << 58));
        for (int k = 1; k < N; k++)
            EXPECT(out[(size_t)k] == 0);
        EXPECT(run(p, alt, 0, out, &nseg) && out[(size_t)N / 2] > (1ull << 59));
        EXPECT(run(p, tone, 0, out, &nseg) && out[5] > (1ull << 59));
        EXPECT(run(p, rnd16, 0, out, &nseg));
        // SC1 and SC8 fill the same range
        std::vector<int16_t> one((size_t)nsamp * 2, -1), m128((size_t)nsamp * 2, -128);
        EXPECT(run(p, one, 2, out, &nseg) && out[0] == 7ull * 2ull * (1ull << 58));
        EXPECT(run(p, m128, 1, out, &nseg) && out[0] == 7ull * 2ull * (1ull << 58));
    }

    // the transform against a DFT in doubles: X[k] = 2^(14 - Wbits) / N * sum of w win e^(-2 pi i k n / N), to a few units
    for (int L : {6, 9}) {
        const int N = 1 << L;
        std::vector<int16_t> w((size_t)N * 2);
        for (auto &v : w)
            v = (int16_t)rnd_in(-20000, 20000);
        gpsbb_psd_t p = plan(L, N, 0, 0);
        for (int n = 0; n < N; n++)
            p.win[n] = (int16_t)rnd_in(-32768, 32767);
        std::vector<uint64_t> out;
        long nseg = 0;
        EXPECT(run(p, w, 0, out, &nseg) && nseg == 1);
        double worst = 0.0;
        for (int k = 0; k < N; k++) {
            double re = 0.0, im = 0.0;
            for (int n = 0; n < N; n++) {
                const double a = -2.0 * M_PI * (double)((long)k * n % N) / N, c = cos(a), s = sin(a), x = (double)w[2 * n] * p.win[n], y = (double)w[2 * n + 1] * p.win[n];
                re += x * c - y * s;
                im += x * s + y * c;
            }
            const double want = (re * re + im * im) / (4.0 * N * N), d = fabs(sqrt((double)out[(size_t)k]) - sqrt(want));
            worst = d > worst ? d : worst;
        }
        EXPECT(worst < 4.0 + L); // every stage rounds twice, by at most a unit in all
    }

    // one call == the sum of a split at a segment boundary; nseg_out may be NULL; refusals write nothing
    {
        const int L = 7, N = 128, hop = 50;
        std::vector<int16_t> w((size_t)(N + 10 * hop + 7) * 2);
        for (auto &v : w)
            v = (int16_t)rnd_in(-32768, 32767);
        gpsbb_psd_t p = plan(L, hop, psd_min_shift(11), 0);
        for (int n = 0; n < N; n++)
            p.win[n] = (int16_t)rnd_in(-32768, 32767);
        std::vector<uint64_t> whole, a, b;
        long nseg = 0, na = 0, nb = 0;
        EXPECT(run(p, w, 0, whole, &nseg) && nseg == 11);
        for (int k : {1, 4, 10}) {
            std::vector<int16_t> first(w.begin(), w.begin() + 2 * (N + (k - 1) * hop)), rest(w.begin() + 2 * k * hop, w.end());
            EXPECT(run(p, first, 0, a, &na) && run(p, rest, 0, b, &nb) && na == k && nb == 11 - k);
            for (int i = 0; i < N; i++)
                EXPECT(a[(size_t)i] + b[(size_t)i] == whole[(size_t)i]);
        }
        std::vector<psd_c> work((size_t)2 * N);
        std::vector<uint64_t> out((size_t)N, 7);
        EXPECT(psd_host(&p, w.data(), (long)w.size() / 2, 0, tc, ts, work.data(), out.data(), nullptr) && out == whole);
        std::fill(out.begin(), out.end(), 7);
        EXPECT(!psd_host(&p, w.data(), N - 1, 0, tc, ts, work.data(), out.data(), &nseg) && !psd_host(&p, nullptr, N, 0, tc, ts, work.data(), out.data(), &nseg));
        EXPECT(!psd_host(&p, w.data(), N, 3, tc, ts, work.data(), out.data(), &nseg) && out[0] == 7 && nseg == 11);
    }
    if (bad)
        return 1;
    printf("psd_asan: table, bound, checks, plans, the range's worst cases, the transform against a DFT, the split: clean\n");
    return 0;
}
