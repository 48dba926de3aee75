// refine_kernels.h - frisk_refine_ranges: the boundaries of a region moved to the base by a likelihood-ratio change point
// (include/frisk_hip.h states the definition, frisk_amd/refine.py restates it in numpy, DESIGN.md section 17 says why it is this
// one).  The row of the range kernels is the region's CORE [a + Fe, b - Fe): the forms and the row loop are range_kernels.h's own
// (ShortForm, LongForm, range_row_loop) and count it as frisk_score_ranges counts a slice; one mode (RefineMode) on either form
// then does, with the core's tables of order r + 1 still in place:
//
//   table   qtab(c) = lp(n_i(c), T_i(c >> 2)) - lp(n_h(c), T_h(c >> 2)) of every word of r + 1 letters into LDS when 4^(r+1) <= 1024
//           (8 KB; the default order gives 64 words); above that a base computes its word's value where it stands.  The host side
//           lp(n_h, T_h) is built once per call by refine_host_kernel from the symmetric counts.
//   cuts    both search intervals are sequences x_0 .. x_{n-1} of per-base values (the start cut's read backwards from a + Fe - 1,
//           the stop cut's forwards from b - Fe) and both ask for the SHORTEST prefix of maximal sum: thread t sums the segment
//           [t * seg, (t + 1) * seg) and keeps its best prefix; the segments' (sum, best, where) combine associatively, in order -
//           over the wave by cross-lane moves, over the workgroup through NW entries of LDS.  A tie goes to the earlier prefix in
//           every combination, so the answer is the shortest region of maximal likelihood ratio, a function of the sequence alone.
//
// Integer arithmetic only: flog2 is 32 squarings of a Q1.63 mantissa, every sum an exact int64 (|q| < 2^39, at most 2^17 bases).
// No floating-point operation, no atomic on an output.
#pragma once
#include "frisk_hip.h"
#include "range_kernels.h"
#include "refine_math.h"

#define FRISK_REFINE_LDS_ORDER 5        // words of up to this many letters have their qtab in LDS

struct RefineParams {
    RangeParams R;              // ranges: the cores
    const int64_t* geom;        // per caller's row, FRISK_REFINE_GEOM entries: resident position of the scaffold's first base, a, b, Fe,
                                // bases searched left of a, bases searched right of b
    const int64_t* host_lp;     // lp(n_h(c), T_h(c >> 2)) of the 4^(order+1) words
    int32_t order;              // r
    // outputs, indexed by the caller's row
    int64_t* new_start;
    int64_t* new_stop;
    int64_t* gain_start;
    int64_t* gain_stop;
    int64_t* flank_used;
};

// the host side of qtab, once per call; sym: the symmetric counts of order r + 1
__global__ void refine_host_kernel(const int64_t* __restrict__ sym, int64_t n_words, int64_t* __restrict__ host_lp) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t c = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; c < n_words; c += step) {
        const int64_t* four = sym + (c & ~int64_t(3));
        host_lp[c] = refine_lp(uint64_t(sym[c]), uint64_t(four[0]) + uint64_t(four[1]) + uint64_t(four[2]) + uint64_t(four[3]));
    }
}

__device__ inline int64_t refine_shfl_xor(int64_t v, int d) {
    const uint32_t hi = uint32_t(__shfl_xor(int(uint32_t(uint64_t(v) >> 32)), d, 64));
    const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(uint64_t(v))), d, 64));
    return int64_t((uint64_t(hi) << 32) | lo);
}
// the wave's 64 runs joined in lane order, in every lane.  PRECONDITION: all 64 lanes active.
__device__ inline RefineCut refine_wave_join(RefineCut x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        RefineCut y;
        y.sum = refine_shfl_xor(x.sum, d);
        y.best = refine_shfl_xor(x.best, d);
        y.ref = refine_shfl_xor(x.ref, d);
        y.arg = __shfl_xor(x.arg, d, 64);
        x = (lane & d) ? refine_join(y, x) : refine_join(x, y);     // the lane's block of d runs and its neighbour's, in order
    }
    return x;
}

// LDS of the mode: the waves' runs of a cut, the table
template <int NW>
struct RefineLds {
    int64_t sum[NW], best[NW], ref[NW];
    int32_t arg[NW];
    int64_t qtab[1 << (2 * FRISK_REFINE_LDS_ORDER)];
};

// One cut, every thread of the workgroup: the shortest prefix of x_0 .. x_{n-1} with the largest sum (the empty prefix, of sum 0,
// included) - its length `arg`, its sum `best` - and `ref`, the sum of the first Fe values.  n is workgroup-uniform.  Ends behind a
// barrier: X may be rewritten.
template <int NT, typename XOF>
__device__ inline void refine_cut(int32_t n, int32_t Fe, RefineLds<NT / 64>& X, XOF&& x_of, int64_t& best, int32_t& arg, int64_t& ref) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x;
    RefineCut c = refine_run(n, int32_t(tid), NT, Fe, x_of);
    c = refine_wave_join(c);
    if ((tid & 63) == 0) { X.sum[tid >> 6] = c.sum; X.best[tid >> 6] = c.best; X.ref[tid >> 6] = c.ref; X.arg[tid >> 6] = c.arg; }
    __syncthreads();
    RefineCut t = {X.sum[0], X.best[0], X.ref[0], X.arg[0]};
#pragma unroll
    for (int v = 1; v < NW; ++v) t = refine_join(t, RefineCut{X.sum[v], X.best[v], X.ref[v], X.arg[v]});
    __syncthreads();
    refine_pick(t, best, arg);
    ref = t.ref;
}

// ---- the mode ---------------------------------------------------------------------------------------------------------------
// the table and both cuts of one row whose core's tables are ready (a mode of range_row_loop), on either form
template <int NW>
struct RefineMode {
    const RefineParams& E;
    RefineLds<NW>& X;

    __device__ void unrefined(int64_t row, int64_t fe) const {
        const int64_t* G = E.geom + FRISK_REFINE_GEOM * row;
        E.new_start[row] = G[1];
        E.new_stop[row] = G[2];
        E.gain_start[row] = 0;
        E.gain_stop[row] = 0;
        E.flank_used[row] = fe;
    }
    // a core the N rule drops, behind range_write_unresolved
    __device__ void dropped(int64_t row) const {
        if (threadIdx.x == 0) unrefined(row, E.geom[FRISK_REFINE_GEOM * row + 3]);
    }
    template <typename FORM>
    __device__ void score(const FORM& form, int64_t row, uint32_t status, uint32_t, const double*) const {
        constexpr int NT = FORM::NT;
        static_assert(NT == NW * 64, "the form's workgroup");
        const RangeParams& P = E.R;
        const int tid = threadIdx.x;
        const int64_t* G = E.geom + FRISK_REFINE_GEOM * row;
        const int64_t off = G[0], a = G[1], b = G[2];
        const int32_t Fe = int32_t(range_uni(uint32_t(G[3])));
        const int32_t left = int32_t(range_uni(uint32_t(G[4]))), right = int32_t(range_uni(uint32_t(G[5])));
        if (tid == 0) P.status[row] = status;               // (nn: the form's composition wrote it)
        if (Fe == 0) {                                      // fewer than four bases: nothing to search (scalar branch)
            if (tid == 0) unrefined(row, 0);
            __syncthreads();
            return;
        }
        const int r = E.order, x = r + 1;
        const bool in_lds = x <= FRISK_REFINE_LDS_ORDER;    // (a kernel argument: scalar)
        auto qvalue = [&](uint32_t code) -> int64_t {
            const uint32_t first = code & ~3u;
            const uint64_t n = form.count(x, code);
            const uint64_t T = uint64_t(form.count(x, first)) + form.count(x, first + 1) + form.count(x, first + 2) + form.count(x, first + 3);
            return refine_lp(n, T) - E.host_lp[code];
        };
        if (in_lds) {
            for (uint32_t c = tid; c < (1u << (2 * x)); c += NT) X.qtab[c] = qvalue(c);
            __syncthreads();
        }
        // q_j of the scaffold's base j: its word is bases [j - r, j]; never across the scaffold's first base (j < r), never across
        // its last (a PAD is invalid)
        auto q_at = [&](int64_t j) -> int64_t {
            if (j < r) return 0;
            const int64_t g = off + j - r;
            const uint32_t c24 = fetch_codes24(P.codes, g);
            const uint32_t inv16 = fetch_mask16(P.inv, g);
            if (lead_clear16(inv16) < x) return 0;
            const uint32_t code = c24 >> (24 - 2 * x);
            return in_lds ? X.qtab[code] : qvalue(code);
        };
        // the start cut reads backwards from a + Fe - 1 (prefix k = the cut t = a + Fe - k), the stop cut forwards from b - Fe
        // (prefix k = the cut u = b - Fe + k); one body for both, so that the word's value is evaluated at one place
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const int64_t j0 = side ? b - Fe : a + Fe - 1, dj = side ? 1 : -1;
            int64_t best, ref;
            int32_t arg;
            refine_cut<NT>(Fe + (side ? right : left), Fe, X, [&](int32_t i) { return q_at(j0 + dj * i); }, best, arg, ref);
            if (tid == 0) {
                (side ? E.new_stop : E.new_start)[row] = side ? b - Fe + arg : a + Fe - arg;
                (side ? E.gain_stop : E.gain_start)[row] = best - ref;
            }
        }
        if (tid == 0) E.flank_used[row] = Fe;
        // (refine_cut's last barrier: every read of the tables and of X is done)
    }
};

template <bool K8>
__global__ __launch_bounds__(FRISK_RANGE_NT) void refine_short_kernel(const RefineParams E) {
    constexpr int NW = FRISK_RANGE_NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint32_t tl[8];
    __shared__ RefineLds<NW> X;
    ShortForm<K8> form(E.R, lds, tl);
    range_row_loop(E.R, form, RefineMode<NW>{E, X});
}

__global__ __launch_bounds__(FRISK_RANGE_BIG_NT) void refine_long_kernel(const RefineParams E, uint32_t* __restrict__ big, int64_t big_stride) {
    constexpr int NW = FRISK_RANGE_BIG_NT / 64;
    __shared__ uint32_t tl[8];
    __shared__ RefineLds<NW> X;
    LongForm form(E.R, big, big_stride, tl);
    range_row_loop(E.R, form, RefineMode<NW>{E, X});
}
