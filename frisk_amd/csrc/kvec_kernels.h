// kvec_kernels.h - symmetric k-mer proportion vectors of arbitrary ranges of the resident batch (frisk_window_vectors): the reference's
// computeKmers(sym=True, pcaMode=True) -> scrubMirrors -> flattenKmerMap(prop=True) (L280-367, L797-831) for one range per workgroup.
//
//   count  every order x of a..b directly: the word of x bases starting at position j of the range counts when j + x <= length and none
//          of its bases has `inv` set (lowercase counts: the reference upper-cases a window, L334-341).  A word never reaches past the
//          range's last base, whatever follows it in the scaffold.  Forward counts in 32-bit LDS counters, profile layout a..b.
//   fold   kept code c (c <= revcomp(c), canonical order): sym = f[c] + f[rc(c)] - a palindrome gets 2 f[c], the reference's two
//          increments of one key (L350-351).  The kept codes come as a table of counter indices, built once per call on the host.
//   prop   double(sym) / double(S_x), S_x the integer sum of the kept sym of order x: ONE IEEE division per entry (no reciprocal),
//          bit for bit the host's kept.astype(float64) / float(sum).  S_x = 0: status bit 0 and bit FRISK_KVEC_ORDER_SHIFT + x, and
//          the order's entries are written as 0.
//   nn     positions of the range with inv | low set: the reference's countN (anything that is not uppercase A/T/G/C).
#pragma once
#include "frisk_device.h"
#include "frisk_hip.h"          // FRISK_KVEC_*

struct KvecShape {
    int a, b;                   // orders
    int nprof;                  // counters: table_offset(a, b + 1)
    int feat0[FRISK_KVEC_MAX_K + 2];   // feat0[x]: first feature of order x in a row; feat0[b + 1] = F
};

// sum of v over the workgroup's waves into *dst (an LDS word, zeroed and fenced by the caller)
__device__ inline void kvec_block_add(unsigned long long v, unsigned long long* dst) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// ranges: n pairs (padded position of the first base, length >= 1, < 2^32); pairs: 2 F counter indices (c, rc(c)) per kept code.
// X: rows [0, n) of n x F; nn / status: n entries.  Dynamic LDS: shape.nprof counters.
__global__ __launch_bounds__(FRISK_KVEC_THREADS) void kvec_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ inv,
                                                                  const uint32_t* __restrict__ low, const int64_t* __restrict__ ranges,
                                                                  int64_t n, KvecShape shape, const uint32_t* __restrict__ pairs,
                                                                  double* __restrict__ X, int64_t* __restrict__ nn,
                                                                  uint32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t kvec_cnt[];
    __shared__ unsigned long long sums[FRISK_KVEC_MAX_K + 2];   // [x]: S_x; [0]: nn
    const int a = shape.a, b = shape.b;
    const int64_t F = shape.feat0[b + 1];
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const int64_t g0 = ranges[2 * r], len = ranges[2 * r + 1];
        for (int i = threadIdx.x; i < shape.nprof; i += FRISK_KVEC_THREADS) kvec_cnt[i] = 0u;
        if (threadIdx.x < FRISK_KVEC_MAX_K + 2) sums[threadIdx.x] = 0ull;
        __syncthreads();
        unsigned long long my_nn = 0;
        for (int64_t j = threadIdx.x; j < len; j += FRISK_KVEC_THREADS) {
            const int64_t g = g0 + j;
            const uint32_t m8 = fetch_mask8(inv, g);
            my_nn += (m8 >> 7) | fetch_mask1(low, g);
            int run = lead_clear8(m8);                          // valid bases from g on, 8 at the most
            const int64_t left = len - j;                       // bases from g to the range's end
            if (left < run) run = int(left);
            if (run < a) continue;
            const uint32_t c16 = fetch_codes16(codes, g);
            const int top = run < b ? run : b;
            for (int x = a; x <= top; ++x) atomicAdd(&kvec_cnt[int(table_offset(a, x)) + int(c16 >> (16 - 2 * x))], 1u);
        }
        kvec_block_add(my_nn, &sums[0]);
        __syncthreads();
        for (int x = a; x <= b; ++x) {
            unsigned long long s = 0;
            for (int f = shape.feat0[x] + threadIdx.x; f < shape.feat0[x + 1]; f += FRISK_KVEC_THREADS)
                s += (unsigned long long)kvec_cnt[pairs[2 * f]] + kvec_cnt[pairs[2 * f + 1]];
            kvec_block_add(s, &sums[x]);
        }
        __syncthreads();
        uint32_t st = 0;
        for (int x = a; x <= b; ++x) {
            const unsigned long long S = sums[x];
            if (S == 0ull) st |= FRISK_KVEC_EMPTY_ORDER | (1u << (FRISK_KVEC_ORDER_SHIFT + x));
            const double den = double(S);
            for (int f = shape.feat0[x] + threadIdx.x; f < shape.feat0[x + 1]; f += FRISK_KVEC_THREADS) {
                const unsigned long long sym = (unsigned long long)kvec_cnt[pairs[2 * f]] + kvec_cnt[pairs[2 * f + 1]];
                X[r * F + f] = S ? double(sym) / den : 0.0;
            }
        }
        if (threadIdx.x == 0) {
            nn[r] = int64_t(sums[0]);
            status[r] = st;
        }
        __syncthreads();            // the counters and sums are cleared for the next range only after every read of them
    }
}
