// null_kernels.h - null sequences drawn on the device from the Markov chain of the context's finalised profile (frisk_seq_null).
//
// The chain of order r reads the symmetric counts of order r + 1 as they lie in d_sym: context c in [0, 4^r) - the r bases before
// a position, first base most significant, A, T, G, C = 0..3 - continues with base b in proportion to sym_{r+1}[4c + b].  Every base
// is a pure function of (profile, order, seed, sequence index, position): a sequence is cut into blocks of NULL_BLOCK bases, each
// block starts its own generator from a hash of (seed, sequence, block) with context 0 and throws away NULL_BURN steps before its
// first base, so generation is parallel over blocks and a sequence is a prefix of every longer one of the same index.
// frisk_amd/nullmodel.py restates the definition in numpy and produces the same bytes.
//
// One thread per block, as synth_kernel.h: a block is a chain of 4 160 dependent steps (hash, one 32-byte read of the context's
// row, a 64 x 64 -> high 64 multiply, three compares), latency-bound on the row's read; all blocks of all sequences of a batch run
// in one launch.  The table is 32 bytes per context (512 KB at order 7): it stays in L2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "synth_kernel.h"           // synth_mix, SYNTH_GOLDEN

#define NULL_BLOCK 4096
#define NULL_BURN 64                // steps a block discards before its first base: nine times the longest context (7 bases)
#define NULL_SALT 12ull             // (synth_kernel.h's unit hashes use salts 1 .. 11)

// cum[4c + b] = sum_{b' <= b} sym[4c + b'], sym = the profile's table of order r + 1: n_ctx = 4^r rows of four, cum[4c + 3] = T(c)
__global__ __launch_bounds__(256) void null_table_kernel(const int64_t* __restrict__ sym, int64_t n_ctx, uint64_t* __restrict__ cum) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; c < n_ctx; c += stride) {
        uint64_t s = 0;
        for (int b = 0; b < 4; ++b) {
            s += uint64_t(sym[4 * c + b]);
            cum[4 * c + b] = s;
        }
    }
}

// the generator's state at the start of block `blk` of sequence `seq`
__host__ __device__ inline uint64_t null_block_state(uint64_t seed, uint32_t seq, uint64_t blk) {
    return synth_mix(seed ^ synth_mix((uint64_t(seq) << 40) ^ blk ^ (NULL_SALT << 56)));
}

// Flat block g of the batch belongs to the sequence s with blk0[s] <= g < blk0[s + 1] (blk0: n_seq + 1 entries, the running count
// of blocks; an empty sequence has none).  Sequence s lies at out[off[s] .. off[s] + len[s]).  ctx_mask = 4^r - 1.
__global__ __launch_bounds__(64) void null_kernel(uint8_t* __restrict__ out, const int64_t* __restrict__ blk0,
                                                   const int64_t* __restrict__ off, const int64_t* __restrict__ len, int32_t n_seq,
                                                   const uint64_t* __restrict__ cum, uint32_t ctx_mask, uint64_t seed) {
    const int64_t n_blocks = blk0[n_seq];
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n_blocks; g += stride) {
        int32_t lo = 0, hi = n_seq;                 // the last s with blk0[s] <= g: the one that owns g (empty ones before it tie)
        while (hi - lo > 1) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (blk0[mid] <= g) lo = mid; else hi = mid;
        }
        const int64_t blk = g - blk0[lo];
        const int64_t base = blk * NULL_BLOCK;
        const int64_t n = (base + NULL_BLOCK < len[lo] ? base + NULL_BLOCK : len[lo]) - base;
        uint8_t* dst = out + off[lo] + base;
        uint64_t state = null_block_state(seed, uint32_t(lo), uint64_t(blk));
        uint32_t ctx = 0;
        for (int64_t t = -NULL_BURN; t < n; ++t) {
            state += SYNTH_GOLDEN;
            const uint64_t x = synth_mix(state);
            const ulonglong2* row = reinterpret_cast<const ulonglong2*>(cum + 4 * size_t(ctx));
            const ulonglong2 c01 = row[0], c23 = row[1];
            uint32_t b;
            if (c23.y == 0) {                       // a context the profile never saw: uniform
                b = uint32_t(x >> 62);
            } else {
                const uint64_t u = __umul64hi(x, c23.y);
                b = uint32_t(u >= c01.x) + uint32_t(u >= c01.y) + uint32_t(u >= c23.x);
            }
            ctx = ((ctx << 2) | b) & ctx_mask;
            if (t >= 0) dst[t] = uint8_t("ATGC"[b]);
        }
    }
}
