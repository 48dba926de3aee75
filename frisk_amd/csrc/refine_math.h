// refine_math.h - the integer arithmetic of frisk_refine_ranges that does not need a device: the fixed-point logarithm and the
// associative combination of the change-point search (refine_kernels.h uses both; tools/exp/san_host.cpp runs them on a CPU).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FRISK_HD __host__ __device__
#else
#define FRISK_HD
#endif

// high 64 bits of a 128-bit product
FRISK_HD inline uint64_t refine_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return uint64_t((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// 2^32 log2 x from below, 1 <= x < 2^63: x = m 2^e, m in Q1.63; squaring m doubles its logarithm, and the bit that the square
// carries beyond 2 is the fraction's next bit.  Truncation only lowers m: 0 <= 2^32 log2 x - flog2(x) < 1 + 2^-20.
FRISK_HD inline int64_t refine_flog2(uint64_t x) {
    const int e = 63 - __builtin_clzll(x);
    uint64_t m = x << (63 - e);
    uint32_t f = 0;
#if defined(__HIPCC__)
#pragma unroll 1       // one copy of the loop per call site: the long form has 128 VGPRs
#endif
    for (int i = 0; i < 32; ++i) {
        const uint64_t hi = refine_mulhi(m, m), lo = m * m;
        f <<= 1;
        if (hi >> 63) { f |= 1u; m = hi; }
        else m = (hi << 1) | (lo >> 63);
    }
    return (int64_t(e) << 32) + int64_t(f);
}
// Laplace-smoothed log-probability of a word seen n times among T of its context
FRISK_HD inline int64_t refine_lp(uint64_t n, uint64_t T) { return refine_flog2(n + 1) - refine_flog2(T + 4); }

// What a run of consecutive values says about the search: its sum, the largest sum of one of its non-empty prefixes and where that
// prefix ends (the number of values of the whole sequence up to there; -1: an empty run), and the sum of its values in front of Fe.
struct RefineCut {
    int64_t sum, best, ref;
    int32_t arg;
};
// a then b; a tie stays with a: the shorter prefix
FRISK_HD inline RefineCut refine_join(const RefineCut& a, const RefineCut& b) {
    RefineCut c = a;
    if (b.arg >= 0 && (a.arg < 0 || a.sum + b.best > a.best)) { c.best = a.sum + b.best; c.arg = b.arg; }
    c.sum = a.sum + b.sum;
    c.ref = a.ref + b.ref;
    return c;
}

// The run of thread t of nt over a sequence of n values x_of(0) .. x_of(n - 1): the values [t * seg, (t + 1) * seg) that exist,
// seg = ceil(n / nt).  Fe: the values in front of it go to `ref`.
template <typename XOF>
FRISK_HD inline RefineCut refine_run(int32_t n, int32_t t, int32_t nt, int32_t Fe, XOF&& x_of) {
    const int32_t seg = (n + nt - 1) / nt;
    const int32_t s0 = t * seg < n ? t * seg : n, s1 = s0 + seg < n ? s0 + seg : n;
    RefineCut c = {0, 0, 0, -1};
    for (int32_t i = s0; i < s1; ++i) {
        const int64_t v = x_of(i);
        c.sum += v;
        if (i < Fe) c.ref += v;
        if (c.arg < 0 || c.sum > c.best) { c.best = c.sum; c.arg = i + 1; }
    }
    return c;
}

// the whole sequence's run against the empty prefix (length 0, sum 0), which keeps a tie
FRISK_HD inline void refine_pick(const RefineCut& t, int64_t& best, int32_t& arg) {
    const bool some = t.arg >= 0 && t.best > 0;
    best = some ? t.best : 0;
    arg = some ? t.arg : 0;
}
