/*
 * gpsbb_interf.h — the per-emitter arithmetic of the interference definition (include/gpsbb.h, gpsbb_interf_t: the definition in
 * full).  Shared by the host function gpsbb_interf_eval and the device kernels (gpsbb_interf.hip.h, gpsbb_despread.hip.h): the
 * statements below are the same on both sides, it compiles as plain C++ too.  Integer arithmetic only, mod 2^64.
 */
#ifndef GPSBB_INTERF_H
#define GPSBB_INTERF_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GPSBB_IHD __host__ __device__ __forceinline__
#else
#define GPSBB_IHD inline
#endif

namespace gpsbb_impl {

constexpr int INTERF_MAX = 4; /* GPSBB_INTERF_MAX */

/* one emitter as the kernels take it */
struct InterfEm {
    uint64_t phase0, F, R; /* as gpsbb_interf_t, two's complement */
    uint64_t Phi;          /* F * P + R * T(P): the phase one whole sweep adds (chirp) */
    uint64_t magP, magG;   /* floor(2^64 / P), floor(2^64 / period): interf_divmod's multipliers (0: not used) */
    uint32_t G;            /* level_q16 */
    uint32_t P;            /* samples per sweep; 0: a CW emitter */
    uint32_t period;       /* the gate's period; 0: continuous (a gate that is never off is stored as continuous) */
    uint32_t on, offset;
    uint32_t m0, g0;       /* of the launch's first sample s0: s0 mod P, (s0 + offset) mod period ... */
    uint32_t _pad;
    uint64_t k0;           /* ... and s0 div P */
};

struct InterfArgs {
    int n;                      /* emitters, 0 .. INTERF_MAX */
    int shift;                  /* step 4's shift, 0..7 */
    unsigned long long sample0; /* stream position of the launch's first sample (s0) */
    InterfEm e[INTERF_MAX];
};

GPSBB_IHD uint64_t interf_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

/* x = q * d + r with 0 <= r < d, for d >= 2 and mag = floor(2^64 / d), any x: mulhi(x, mag) is q or q - 1, because
 * x * mag / 2^64 falls short of x / d by x * (2^64 / d - mag) / 2^64 < 1.  One fix-up, no division. */
GPSBB_IHD void interf_divmod(uint64_t x, uint32_t d, uint64_t mag, uint64_t *q, uint32_t *r)
{
    uint64_t qq = interf_mulhi(x, mag);
    uint64_t rr = x - qq * (uint64_t)d;
    if (rr >= (uint64_t)d) {
        rr -= (uint64_t)d;
        qq++;
    }
    *q = qq;
    *r = (uint32_t)rr;
}

/* T(x) = x * (x - 1) / 2, exact for x < 2^32 */
GPSBB_IHD uint64_t interf_tri(uint32_t x)
{
    return x ? ((uint64_t)x * (uint64_t)(x - 1u)) >> 1 : 0ull;
}

/* where an emitter is at the sample d samples after the launch's first: phase, the step to the next sample, position in the
 * sweep, position in the gate's period */
struct InterfPos {
    uint64_t theta, inc;
    uint32_t m, g;
};

GPSBB_IHD InterfPos interf_seek(const InterfEm &e, uint64_t s0, uint64_t d)
{
    InterfPos p;
    if (e.P) {
        uint64_t q;
        interf_divmod((uint64_t)e.m0 + d, e.P, e.magP, &q, &p.m);
        p.inc = e.F + e.R * (uint64_t)p.m;
        p.theta = e.phase0 + (e.k0 + q) * e.Phi + e.F * (uint64_t)p.m + e.R * interf_tri(p.m);
    } else {
        p.m = 0u;
        p.inc = e.F;
        p.theta = e.phase0 + e.F * (s0 + d);
    }
    p.g = 0u;
    if (e.period) {
        uint64_t q;
        interf_divmod((uint64_t)e.g0 + d, e.period, e.magG, &q, &p.g);
    }
    return p;
}

/* the emitter's value at p added to (jI, jQ), then p moved on by one sample.  cs(idx, &c, &s) reads the carrier tables.
 * The sawtooth is phase-continuous, so the step F + R * m serves at a sweep's last sample too: T(P) = T(P - 1) + P - 1. */
template <class Tab>
GPSBB_IHD void interf_step(const InterfEm &e, InterfPos &p, const Tab &cs, int &jI, int &jQ)
{
    if (!e.period || p.g < e.on) {
        int c, s;
        cs((uint32_t)(p.theta >> 55), &c, &s);
        jI += (int)(((int64_t)e.G * (int64_t)c + 32768) >> 16);
        jQ += (int)(((int64_t)e.G * (int64_t)s + 32768) >> 16);
    }
    p.theta += p.inc;
    if (e.P) {
        p.m++;
        p.inc += e.R;
        if (p.m == e.P) {
            p.m = 0u;
            p.inc = e.F;
        }
    }
    if (e.period) {
        p.g++;
        if (p.g == e.period)
            p.g = 0u;
    }
}

} /* namespace gpsbb_impl */
#endif
