// seq_kernels.h - the kernels of a sequence batch's way onto the device and back: ASCII -> packed, packed -> ASCII, run lists -> bitmap.
// Non-inline __global__ functions: included by frisk_seq.hip alone.
#pragma once
#include "frisk_device.h"

// ------------------------------------------------------------------------------------------------
// ASCII -> (codes, inv, low).  One thread packs 32 consecutive bases (two 16-byte loads, coalesced
// across the wave: 2 KiB of ASCII per wave-instruction pair) and writes two code words + one word of
// each mask.  HBM-bound: 1 B/base read, 0.5 B/base written.
// ------------------------------------------------------------------------------------------------
__device__ inline void classify_byte(uint32_t c, uint32_t& code, uint32_t& inv, uint32_t& low) {
    const uint32_t u = c & 0xDFu;                       // fold ASCII case
    const uint32_t isA = (u == 'A'), isT = (u == 'T'), isG = (u == 'G'), isC = (u == 'C');
    const uint32_t valid = isA | isT | isG | isC;
    code = isT * 1u + isG * 2u + isC * 3u;              // A=0,T=1,G=2,C=3 (reference L70)
    const uint32_t is_pad = (c == FRISK_PAD_BYTE);
    inv = (valid ^ 1u);
    low = (valid & ((c >> 5) & 1u)) | is_pad;           // lowercase acgt, or PAD (inv & low)
}

__global__ __launch_bounds__(256) void pack_kernel(const uint8_t* __restrict__ ascii, int64_t nwords32,
                                                    uint32_t* __restrict__ codes, uint32_t* __restrict__ inv,
                                                    uint32_t* __restrict__ low) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < nwords32; t += stride) {
        const uint4* src = reinterpret_cast<const uint4*>(ascii + t * 32);
        const uint4 q0 = src[0], q1 = src[1];
        const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        uint32_t c0 = 0, c1 = 0, mi = 0, ml = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const uint32_t ch = (w[b >> 2] >> (8 * (b & 3))) & 0xFFu;
            uint32_t code, i1, l1;
            classify_byte(ch, code, i1, l1);
            if (b < 16) c0 |= code << (30 - 2 * b); else c1 |= code << (30 - 2 * (b - 16));
            mi |= i1 << (31 - b);
            ml |= l1 << (31 - b);
        }
        codes[2 * t] = c0;
        codes[2 * t + 1] = c1;
        inv[t] = mi;
        low[t] = ml;
    }
}

// packed -> canonical ASCII (A/T/G/C, a/t/g/c, N; PAD -> '\0'): test / read-back utility
__global__ __launch_bounds__(256) void unpack_kernel(const uint32_t* __restrict__ codes,
                                                      const uint32_t* __restrict__ inv,
                                                      const uint32_t* __restrict__ low, int64_t p0, int64_t n,
                                                      uint8_t* __restrict__ out) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < n; t += stride) {
        const int64_t g = p0 + t;
        const uint32_t i1 = fetch_mask1(inv, g), l1 = fetch_mask1(low, g), c = fetch_code2(codes, g);
        uint8_t ch;
        if (i1 && l1) ch = 0;
        else if (i1) ch = 'N';
        else ch = uint8_t("ATGC"[c] | (l1 ? 0x20 : 0));
        out[t] = ch;
    }
}

// Run lists -> bitmap (the 0.25 B/base upload form, seq_pack2.h): `runs` holds n_runs pairs [begin, end) of padded positions,
// disjoint within one list; every position of a run gets its bit set (position p = bit 31 - (p & 31) of word p >> 5).  One
// wavefront per run: whole words inside a run are plain stores (a word covered entirely by one run belongs to no other run
// of the list), the ragged first / last word an atomic OR (another list - the PADs - may share it).  The bitmap was zeroed
// on the same stream.  HBM-bound at 1 bit per covered position; a list of millions of short runs costs a wave each.
__global__ __launch_bounds__(256) void expand_runs_kernel(const int64_t* __restrict__ runs, int64_t n_runs,
                                                           uint32_t* __restrict__ bits) {
    const int lane = int(threadIdx.x & 63u);
    const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_runs; r += nwaves) {
        const int64_t b = runs[2 * r], e = runs[2 * r + 1];
        if (e <= b) continue;
        const int64_t w0 = b >> 5, w1 = (e - 1) >> 5;
        for (int64_t w = w0 + lane; w <= w1; w += 64) {
            const int64_t lo = w << 5;
            const int from = b > lo ? int(b - lo) : 0, to = e < lo + 32 ? int(e - lo) : 32;      // bits [from, to) of the word
            const uint32_t m = uint32_t((0xFFFFFFFFull >> from) & ~(0xFFFFFFFFull >> to));
            if (m == 0xFFFFFFFFu) bits[w] = m;
            else atomicOr(bits + w, m);
        }
    }
}
