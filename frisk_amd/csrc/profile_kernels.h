// profile_kernels.h - phase A (genome k-mer profile) kernels, included by frisk_abi.hip alone.  (Pack / unpack of scaffolds: seq_kernels.h.)
// Reference semantics: computeKmers(genomeMode=True), frisk/__init__.py L280-367, called at L1442.
#pragma once
#include "frisk_device.h"

// ------------------------------------------------------------------------------------------------
// Phase A counting.  Every padded position p contributes exactly ONE histogram update: to the table
// of order r = min(run, K) at the code of its longest valid word, where run = number of consecutive
// valid bases starting at p (a PAD or an invalid letter stops it; with --maskHost a soft-masked base
// stops it too, L336-337).  Lower orders follow by marginalisation (marginalize_kernel): a valid
// (r)-mer contains a valid x-mer prefix for every x <= r, so
//      C_x[q] = D_x[q] + sum_b C_{x+1}[4q+b]          (C_K = D_K)
// which is exact, including scaffold ends and N-adjacent positions.  `raw` = the D tables (profile
// layout) followed by {totalLen, #K-mer start positions, nnTotal, 0}; everything in it is a plain sum
// over positions, hence summable across batches and across GPUs.
// A lane owns one 32-position WORD of the bitmaps (7 loads: two words of each bitmap, three of the codes); the
// run flags of its 32 positions come from whole-word shifts, the codes from constant shifts, so a position costs
// about ten instructions instead of its own three unaligned fetches.  That walk is written once (load_word,
// run_starts, code_at, add_runs, ProfScalars; walk_words for the forms with a table in LDS); the three kernels
// differ in where a position with a full-length word (run >= K) is counted:
//   profile_add_kernel      32-bit counters in LDS, flushed once with one global atomic per non-empty bin.  4^8 x 4 B =
//                           256 KiB does not fit a CU's 160 KiB, so at K = 8 the k-mer space is split in two halves by the
//                           leading bit of the code and a workgroup makes its pass over its chunk for ONE half (grid =
//                           chunks x halves; the sequence is 0.5 B/base, reading it twice is free);
//   profile_add16_kernel    K = 8: 16-bit fields in LDS, all of 4^8 in one walk;
//   profile_add_big_kernel  K > 8: the global table, like every shorter run.
// Orders below K (positions next to an invalid base or a scaffold end: a vanishing share) go straight to global atomics,
// as do the three scalars (one atomic per wave); of the workgroups that walk a chunk more than once, the first walk alone
// counts those.  Which form a range takes, and its grid: profile_plan.h.
// ------------------------------------------------------------------------------------------------
#define FRISK_PROF_NT 1024

// the resident batch and the positions [p0, p1) of one launch
struct ProfRange {
    const uint32_t* __restrict__ codes;
    const uint32_t* __restrict__ inv;
    const uint32_t* __restrict__ low;
    int64_t p0, p1;
    int mask_host;
    __device__ int64_t w_first() const { return p0 >> 5; }                 // bitmap words that hold [p0, p1)
    __device__ int64_t w_end() const { return (p1 + 31) >> 5; }
    __device__ void chunk(int64_t i, int64_t chunk_words, int64_t& wb, int64_t& we) const {    // the words of chunk i
        wb = w_first() + i * chunk_words;
        we = wb + chunk_words;
        if (we > w_end()) we = w_end();
    }
};

// the k most significant bits of a word (k clamped to 0..32)
__device__ __forceinline__ uint32_t topbits(int64_t k) {
    k = k < 0 ? 0 : (k > 32 ? 32 : k);
    return uint32_t(0xFFFFFFFF00000000ull >> k);
}

// One 32-position word of the bitmaps as its lane sees it.  Position base+j (base = 32 wq) is bit 31-j of a 32-bit mask and
// bit 63-j of a 64-bit one, whose low half is the next word's positions: what a run that starts in this word can reach.
struct ProfWord {
    uint32_t inr;           // positions of the word inside [p0, p1)
    uint32_t other;         // not an uppercase A/T/G/C (countN, L106-118)
    uint64_t V;             // countable bases: valid, and under --maskHost not soft-masked
    uint64_t NP;            // not a PAD
    uint64_t lo64, hi64;    // the codes from position base on, and from base+16 on
};

__device__ __forceinline__ ProfWord load_word(const ProfRange& r, int64_t wq) {
    const int64_t base = wq << 5;                                           // position of bit 31 of this word
    const uint32_t i0 = r.inv[wq], i1 = r.inv[wq + 1], l0 = r.low[wq], l1 = r.low[wq + 1];
    const uint32_t c0 = r.codes[2 * wq], c1 = r.codes[2 * wq + 1], c2 = r.codes[2 * wq + 2];
    const uint32_t e0 = i0 | (r.mask_host ? l0 : 0u), e1 = i1 | (r.mask_host ? l1 : 0u);
    ProfWord W;
    W.inr = topbits(r.p1 - base) & ~topbits(r.p0 - base);
    W.other = i0 | l0;
    W.V = ~((uint64_t(e0) << 32) | e1);
    W.NP = ~((uint64_t(i0 & l0) << 32) | (i1 & l1));
    W.lo64 = (uint64_t(c0) << 32) | c1;
    W.hi64 = (uint64_t(c1) << 32) | c2;
    return W;
}

// The positions that start a run of k set bits of M.  K8: k is 8, in three doubling steps.
template <bool K8>
__device__ __forceinline__ uint64_t run_starts(uint64_t M, int k) {
    uint64_t F = M;
    if (K8) { F &= F << 1; F &= F << 2; F &= F << 4; }
    else for (int s = 1; s < k; ++s) F &= M << s;
    return F;
}

// BITS (16, or 24 for the orders above 8) of code from position j of the word on; by constant shifts where j is a constant
template <int BITS>
__device__ __forceinline__ uint32_t code_at(const ProfWord& W, int j) {
    return uint32_t((j < 16 ? W.lo64 : W.hi64) >> (64 - BITS - 2 * (j & 15))) & ((1u << BITS) - 1u);
}

// The positions `todo` of a word (countable ones) straight to the global tables: each to the table of order run = min(its run, kmax),
// when that is an order of the profile.  For the forms with a table in LDS these are the few positions whose run is shorter than kmax.
template <int BITS>
__device__ __forceinline__ void add_runs(const ProfWord& W, uint32_t todo, int kmin, int kmax, unsigned long long* __restrict__ raw) {
    while (todo) {
        const int j = __clz(int(todo));
        todo &= ~(0x80000000u >> j);                                        // (clears the top bit)
        int run = __clzll((long long)(~(W.V << j)));                        // countable bases from here on (<= 32 visible)
        run = run < kmax ? run : kmax;
        if (run >= kmin) atomicAdd(&raw[table_offset(kmin, run) + (code_at<BITS>(W, j) >> (BITS - 2 * run))], 1ull);
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {     // lane 0 of each wave holds the wave's sum
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// The three scalars of raw's tail, summed by a lane over its words; flush(): one atomic per wave and scalar
struct ProfScalars {
    unsigned long long tot = 0, kpos = 0, nn = 0;
    template <bool K8>
    __device__ __forceinline__ void add(const ProfWord& W, int kmax) {
        const uint64_t G = run_starts<K8>(W.NP, kmax);                      // a K-mer can start here (L329): no PAD in reach
        const uint32_t real = uint32_t(W.NP >> 32) & W.inr;
        tot += __popc(real);
        nn += __popc(real & W.other);
        kpos += __popc(uint32_t(G >> 32) & W.inr);
    }
    __device__ __forceinline__ void flush(unsigned long long* __restrict__ tail) {     // tail = raw + nprof; all lanes of the wave call
        tot = wave_sum(tot);
        kpos = wave_sum(kpos);
        nn = wave_sum(nn);
        if ((threadIdx.x & 63) == 0) {
            if (tot) atomicAdd(&tail[0], tot);
            if (kpos) atomicAdd(&tail[1], kpos);
            if (nn) atomicAdd(&tail[2], nn);
        }
    }
};

// A workgroup's table of `nwords` 32-bit words in LDS: zeroed, and (as 32-bit counters) added to the global bins dst[0 .. nwords)
__device__ __forceinline__ void clear_table(uint32_t* hist, uint32_t nwords) {
    for (uint32_t b = threadIdx.x; b < nwords / 4; b += blockDim.x) reinterpret_cast<uint4*>(hist)[b] = make_uint4(0, 0, 0, 0);
    if (nwords < 4) for (uint32_t b = threadIdx.x; b < nwords; b += blockDim.x) hist[b] = 0;
}
__device__ __forceinline__ void flush_table32(const uint32_t* hist, uint32_t nbins, unsigned long long* __restrict__ dst) {
    for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x) {
        const uint32_t v = hist[b];
        if (v) atomicAdd(&dst[b], (unsigned long long)v);
    }
}

// Where the two-half form counts a full-length word: in the 32-bit counter of its code, if the code's leading bit is this half's
// (one half: every code).  The bins of half h are raw[offK + h * nbins ...].
struct HalfTable {
    uint32_t* hist;
    uint32_t nbins, halfbit, mine;
    int shK;
    __device__ __forceinline__ HalfTable(uint32_t* hist_, int kmax, int halves, int half)
        : hist(hist_), nbins((1u << (2 * kmax)) / uint32_t(halves)), halfbit(halves == 2 ? nbins : 0u), mine(half ? halfbit : 0u),
          shK(16 - 2 * kmax) {}
    __device__ __forceinline__ void operator()(uint32_t c16) const {
        const uint32_t code = c16 >> shK;
        if ((code & halfbit) == mine) atomicAdd(&hist[code & (nbins - 1)], 1u);
    }
};

// One walk of a workgroup over the words [wb, we), a lane a word: every position that starts a full-length word goes to full(16
// bits of code, of which the leading 2 kmax are that word); with `rest`, everything that bypasses the table as well - the shorter
// runs and the three scalars.  -> (rest) the full-length positions this lane counted.
template <bool K8, class Full>
__device__ __forceinline__ unsigned long long walk_words(const ProfRange& r, int64_t wb, int64_t we, int kmin, int kmax, bool rest,
                                                         unsigned long long* __restrict__ raw, int nprof, const Full& full) {
    ProfScalars S;
    unsigned long long counted = 0;
    for (int64_t wq = wb + threadIdx.x; wq < we; wq += blockDim.x) {
        const ProfWord W = load_word(r, wq);
        const uint64_t F = run_starts<K8>(W.V, kmax);                       // ... that start a run of kmax countable bases
        const uint32_t fullm = uint32_t(F >> 32) & W.inr;
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (fullm & (0x80000000u >> j)) full(code_at<16>(W, j));
        if (rest) {
            counted += uint32_t(__popc(fullm));
            add_runs<16>(W, uint32_t(W.V >> 32) & ~uint32_t(F >> 32) & W.inr, kmin, kmax, raw);
            S.add<K8>(W, kmax);
        }
    }
    if (rest) S.flush(raw + nprof);
    return counted;
}

// kmax <= 8: the order-K table privatised per workgroup as 32-bit counters, in one or (K = 8) two halves.  Half 0 alone counts
// what bypasses the table.
__global__ __launch_bounds__(FRISK_PROF_NT) void profile_add_kernel(const uint32_t* __restrict__ codes,
                                                                     const uint32_t* __restrict__ inv,
                                                                     const uint32_t* __restrict__ low, int64_t p0, int64_t p1,
                                                                     int kmin, int kmax, int mask_host, int nprof,
                                                                     int halves, int64_t chunk_words,
                                                                     unsigned long long* __restrict__ raw) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
    const int half = int(blockIdx.x) % halves;
    const HalfTable table(hist, kmax, halves, half);
    clear_table(hist, table.nbins);
    __syncthreads();
    const ProfRange r{codes, inv, low, p0, p1, mask_host};
    int64_t wb, we;
    r.chunk(int64_t(blockIdx.x) / halves, chunk_words, wb, we);
    walk_words<false>(r, wb, we, kmin, kmax, half == 0, raw, nprof, table);
    __syncthreads();
    flush_table32(hist, table.nbins, raw + table_offset(kmin, kmax) + uint32_t(half) * table.nbins);
}

// K = 8 in ONE pass (round 4): the order-8 table as 4^8 SIXTEEN-bit counters, two to a word = 128 KiB, so that a workgroup
// counts every max-mer of its chunk in one walk instead of making the walk once per half of the k-mer space (the walk - masks,
// run flags, code extraction: ~10 instructions per position - is what the kernel's time is; the two-half form did it twice).
// A 16-bit field can wrap (65 536 copies of one 8-mer inside one workgroup's chunk: a megabase of poly-A), and a wrap is
// found the way the scan kernels find theirs: the table's grand total must equal the number of max-mer positions the
// workgroup counted.  It never does in assemblies; where it does, the workgroup throws its table away and counts its chunk
// again in the two-half form, one half after the other (32-bit counters in the same LDS).  Everything that does not go through
// the table - short runs, the three scalars - is added to the global tables during the first walk only.
__global__ __launch_bounds__(FRISK_PROF_NT) void profile_add16_kernel(const uint32_t* __restrict__ codes,
                                                                       const uint32_t* __restrict__ inv,
                                                                       const uint32_t* __restrict__ low, int64_t p0, int64_t p1,
                                                                       int kmin, int mask_host, int nprof, int64_t chunk_words,
                                                                       unsigned long long* __restrict__ raw) {
    constexpr int K = 8;
    constexpr uint32_t NW = (1u << (2 * K)) / 2;                            // 32 768 words: two 16-bit counters each, or one half's 32-bit counters
    extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
    __shared__ unsigned long long red[2];                                   // max-mer positions counted / the table's grand total
    clear_table(hist, NW);
    if (threadIdx.x < 2) red[threadIdx.x] = 0ull;
    __syncthreads();
    const ProfRange r{codes, inv, low, p0, p1, mask_host};
    int64_t wb, we;
    r.chunk(int64_t(blockIdx.x), chunk_words, wb, we);
    const int64_t offK = table_offset(kmin, K);
    const unsigned long long counted = wave_sum(walk_words<true>(r, wb, we, kmin, K, true, raw, nprof, [&](uint32_t code) {
        atomicAdd(&hist[code >> 1], 1u << ((code & 1u) * 16u));             // every max-mer into its 16-bit field
    }));
    if ((threadIdx.x & 63) == 0 && counted) atomicAdd(&red[0], counted);
    __syncthreads();
    {   // the table's grand total
        unsigned long long sum = 0;
        for (uint32_t b = threadIdx.x; b < NW; b += blockDim.x) { const uint32_t v = hist[b]; sum += (v & 0xFFFFu) + (v >> 16); }
        sum = wave_sum(sum);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&red[1], sum);
    }
    __syncthreads();
    if (red[0] == red[1]) {                 // (uniform) no field wrapped: every counter is what it says
        for (uint32_t b = threadIdx.x; b < NW; b += blockDim.x) {
            const uint32_t v = hist[b];
            if (v & 0xFFFFu) atomicAdd(&raw[offK + 2u * b], (unsigned long long)(v & 0xFFFFu));
            if (v >> 16) atomicAdd(&raw[offK + 2u * b + 1u], (unsigned long long)(v >> 16));
        }
        return;
    }
    for (int half = 0; half < 2; ++half) {  // a wrapped field: the chunk again, half by half, in 32-bit counters and nothing else
        __syncthreads();
        clear_table(hist, NW);
        __syncthreads();
        walk_words<true>(r, wb, we, kmin, K, false, raw, nprof, HalfTable(hist, K, 2, half));
        __syncthreads();
        flush_table32(hist, NW, raw + offK + uint32_t(half) * NW);
    }
}

// The same counting for kmax > 8 (4^K 32-bit counters no longer fit a CU's LDS): every position's ONE update goes straight to
// the global table of its order.  A lane owns one 32-position word of the bitmaps as above; 24-bit codes (12 bases), and a
// grid-stride loop in place of chunks.
// ~20 ms per 400 Mb - the reference's -k is unbounded (L1197-1206) but its own cost grows with 4^K; this path is for
// completeness, not speed.
__global__ __launch_bounds__(256) void profile_add_big_kernel(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ inv,
                                                               const uint32_t* __restrict__ low, int64_t p0, int64_t p1, int kmin,
                                                               int kmax, int mask_host, int nprof,
                                                               unsigned long long* __restrict__ raw) {
    const ProfRange r{codes, inv, low, p0, p1, mask_host};
    ProfScalars S;
    for (int64_t wq = r.w_first() + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; wq < r.w_end(); wq += int64_t(gridDim.x) * blockDim.x) {
        const ProfWord W = load_word(r, wq);
        add_runs<24>(W, uint32_t(W.V >> 32) & W.inr, kmin, kmax, raw);
        S.add<false>(W, kmax);
    }
    S.flush(raw + nprof);
}

// C_x[q] = D_x[q] + sum_b C_{x+1}[4q+b], in place on a copy of the D tables; one launch per order,
// from K-1 down to kmin (4^x threads each).
__global__ __launch_bounds__(256) void marginalize_kernel(int64_t* __restrict__ cnt, int kmin, int x) {
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= (int64_t(1) << (2 * x))) return;
    const int64_t* up = cnt + table_offset(kmin, x + 1) + 4 * q;
    cnt[table_offset(kmin, x) + q] += up[0] + up[1] + up[2] + up[3];
}

// The same for all orders x_hi, x_hi-1, ..., kmin in ONE launch of one workgroup (x_hi <= 7: at most 16 K bins on the widest
// level): below order 8 a launch per order is all launch latency (seven launches of ~2 us of work, ~7 us apart).
__global__ __launch_bounds__(1024) void marginalize_low_kernel(int64_t* __restrict__ cnt, int kmin, int x_hi) {
    for (int x = x_hi; x >= kmin; --x) {
        const int64_t n = int64_t(1) << (2 * x);
        int64_t* dst = cnt + table_offset(kmin, x);
        const int64_t* up = cnt + table_offset(kmin, x + 1);
        for (int64_t q = threadIdx.x; q < n; q += blockDim.x) dst[q] += up[4 * q] + up[4 * q + 1] + up[4 * q + 2] + up[4 * q + 3];
        __threadfence_block();
        __syncthreads();
    }
}

// genome mode adds the reverse complement of every counted word (L350-351):
// sym[c] = fwd[c] + fwd[rc(c)] - a palindromic word therefore counts twice per occurrence.
__global__ __launch_bounds__(256) void symmetrize_kernel(const int64_t* __restrict__ fwd, int64_t* __restrict__ sym,
                                                          int kmin, int kmax) {
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (int x = kmin; x <= kmax; ++x) {
        const int64_t off = table_offset(kmin, x), n = int64_t(1) << (2 * x);
        if (t >= off && t < off + n) {
            const uint32_t c = uint32_t(t - off);
            sym[t] = fwd[t] + fwd[off + revcomp_code(c, x)];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Genome-side IVOM value of EVERY max-mer, before normalisation (IvomBuild with isGenomeIVOM=True,
// L411-450).  It depends only on the genome profile, so it is computed once per profile; the scan
// kernel gathers from it and renormalises over the window's present max-mers (L453-454).
// A zero running weight or a zero divisor is a ZeroDivisionError in the reference (L437, L416-424):
// encoded as NaN and reported per window if such a max-mer is present there.  The genome side keeps the
// reference's operation order (it is computed once; the scan kernel uses the closed form on the window side).
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
// metadata of L356-359 on the device: meta[0] = totalLen, meta[1] = exMax = the K-mer start positions that were NOT counted,
// meta[2] = nnTotal.  `cnt` = marginalised forward counts (profile layout), `raw_tail` = {totalLen, K-mer start positions,
// nnTotal} summed over positions.  One workgroup; the order-K table has at most 4^8 entries.
__global__ __launch_bounds__(1024) void profile_meta_kernel(const int64_t* __restrict__ cnt, const int64_t* __restrict__ raw_tail,
                                                             int kmin, int kmax, int64_t* __restrict__ meta) {
    __shared__ long long part[16];
    const int64_t n = int64_t(1) << (2 * kmax);
    const int64_t* top = cnt + table_offset(kmin, kmax);
    long long s = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += top[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long counted = 0;
        for (int w = 0; w < int(blockDim.x >> 6); ++w) counted += part[w];
        meta[0] = raw_tail[0];
        meta[1] = raw_tail[1] - counted;
        meta[2] = raw_tail[2];
    }
}

// `meta` (device): {totalLen, exMax, nnTotal}; genomeSpace = totalLen - nnTotal (L379)
__global__ __launch_bounds__(256) void genome_ivom_kernel(const int64_t* __restrict__ sym, int kmin, int kmax,
                                                           const int64_t* __restrict__ meta, double* __restrict__ ig) {
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= (int64_t(1) << (2 * kmax))) return;
    const int64_t genome_space = meta[0] - meta[2];
    unsigned long long W = 0;
    double I = 0.0;
    bool bad = false;
    for (int x = kmin; x <= kmax; ++x) {
        const int64_t c = sym[table_offset(kmin, x) + (k >> (2 * (kmax - x)))];
        const unsigned long long wt = (unsigned long long)c << (2 * x);
        W += wt;
        const int64_t D = (genome_space - (x - 1)) * 2;
        if (W == 0 || D == 0) { bad = true; break; }
        const double p = double(c) / double(D);
        const double a = double(wt) / double(W);
        I = (x == kmin) ? a * p : a * p + ((1.0 - a) * I);
    }
    ig[k] = bad ? __longlong_as_double(0x7FF8000000000000LL) : I;
}
