// explain_kernels.h - frisk_explain_ranges: the rows of range_kernels.h, and for each the present max-mers that contribute the
// largest summands to its KLD (KLD L465-470: term_k = pw_k * (ln(pw_k / pg_k) / ln 2), the sum over the present max-mers).  A range
// is counted once - the forms and the row loop are range_kernels.h's own (ShortForm, LongForm, range_row_loop) - and scored twice,
// by one mode (ExplainMode) on either form:
//
//   walk    the order-K table once: the codes of the non-empty bins go to the workgroup's slice of global scratch, compacted by
//           wave ballots (one LDS atomic per wave and step).  Where in the slice a code lands depends on the arrival order of those
//           atomics; nothing below depends on where.  The walk does not score (as panel_kernels.h's: inside the walk the FP64 body
//           would run with a twelfth of its lanes active); both passes run over the slice, one entry per lane, every lane busy.
//   pass 1  range_kernels.h's scoring body on every entry, then range_finish, unchanged: the row's status, kld, gc, pi, si, cri and
//           nn are bit for bit frisk_score_ranges' (ExactSum totals do not depend on which lane scored which max-mer).  It leaves Sw
//           and Sg, the exact sums, in every thread.
//   pass 2  (rows whose status is exactly ROW_KEPT) Iw and Ig of an entry as in range_maxmer_add, pw = Iw / Sw, pg = Ig / Sg,
//           term = pw * (ln(pw / pg) / ln 2) - the reference's expression in its order - stored beside the entry's code.
//   select  top_n rounds of a workgroup arg-max over the total order (term descending as numbers - -0.0 equals +0.0 -, code
//           ascending).  Every thread keeps the first entry, in that order, of its share of the slice (entries tid, tid + NT, ... -
//           the ones it scored) behind the previous winner; a round reduces these candidates over the wave by cross-lane moves and
//           over the workgroup through 2 x NW entries of LDS (double-buffered: one barrier per round), and only the share of the
//           thread that owned the winner is looked through again - by its whole wave.  The winner of a round is the first of the set's entries behind the
//           previous winner: a function of the set of (term, code) pairs alone - not of the lanes, the form, the grid or the other
//           rows.
//   write   thread j < min(top_n, present) evaluates winner j once more - the same operations on the same operands: the same bits -
//           for its count, pw, pg and term.
//
// Every other slot (rows the N rule drops, rows that are not plainly kept, ranks behind the last present max-mer) keeps what
// explain_fill_kernel wrote before the launch.  A slice holds min(longest range of the launch, 4^kmax) entries: a range of n bases
// has at most n - kmax + 1 distinct max-mers; a store is guarded by the capacity all the same.
//
// FP64 throughout, no MFMA, no floating-point atomics.
#pragma once
#include "frisk_hip.h"
#include "range_kernels.h"

#pragma clang fp contract(off)

#define FRISK_EXPLAIN_NONE 0xFFFFFFFFu      // code of an empty slot

struct ExplainParams {
    RangeParams R;
    int32_t top_n;              // 1 .. FRISK_EXPLAIN_MAX
    // outputs: n_present per caller's row; the others [row][top_n], slot j = rank j
    int32_t* n_present;
    uint32_t* code;
    uint32_t* count;
    double* pw;
    double* pg;
    double* term;
    double* stage;              // per workgroup: `cap` terms, then `cap` codes (32-bit)
    int64_t cap;                // entries of a slice, even
};

// the empty slots of a call, before its kernels
__global__ void explain_fill_kernel(const ExplainParams E, int64_t n_rows) {
    const double qnan = __longlong_as_double(0x7FF8000000000000LL);
    const int64_t step = int64_t(gridDim.x) * blockDim.x, slots = n_rows * E.top_n;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < slots; i += step) {
        E.code[i] = FRISK_EXPLAIN_NONE;
        E.count[i] = 0u;
        E.pw[i] = qnan; E.pg[i] = qnan; E.term[i] = qnan;
        if (i < n_rows) E.n_present[i] = 0;
    }
}

// An entry of the selection.  key: the term's bits mapped so that unsigned order is numeric order, both zeros on one key; 0 is
// below every number's key: no entry.
struct ExplainPick {
    unsigned long long key;
    uint32_t code;
};
__device__ inline unsigned long long explain_key(double t) {
    unsigned long long b = (unsigned long long)__double_as_longlong(t);
    if ((b << 1) == 0ull) b = 0ull;                                     // -0.0 -> +0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline ExplainPick explain_none() { return ExplainPick{0ull, FRISK_EXPLAIN_NONE}; }
// a ranks before b: the larger term, then the smaller code
__device__ inline bool explain_before(const ExplainPick& a, const ExplainPick& b) {
    return a.key > b.key || (a.key == b.key && a.code < b.code);
}

// the first of the wave's candidates, in every lane.  PRECONDITION: all 64 lanes active.
__device__ inline ExplainPick explain_wave_first(ExplainPick x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        ExplainPick y;
        const uint32_t hi = uint32_t(__shfl_xor(int(uint32_t(x.key >> 32)), d, 64));
        const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(x.key)), d, 64));
        y.key = ((unsigned long long)hi << 32) | lo;
        y.code = uint32_t(__shfl_xor(int(x.code), d, 64));
        if (explain_before(y, x)) x = y;
    }
    return x;
}

// The first entry that ranks behind `prev` in the share of thread `owner` of the workgroup (entries owner, owner + NT, ...), in
// every lane.  The whole wave looks: lane l takes the share's entries l, l + 64, ... - one round of loads instead of a chain in one
// lane.  PRECONDITION: all 64 lanes active, `owner` wave-uniform; the share's terms were stored before the round's barrier.
template <int NT>
__device__ inline ExplainPick explain_share_next(const double* st, const uint32_t* sc, uint32_t m, uint32_t owner, const ExplainPick& prev) {
    ExplainPick best = explain_none();
    for (uint64_t i = owner + uint64_t(threadIdx.x & 63) * NT; i < m; i += 64u * NT) {
        const ExplainPick x = {explain_key(st[i]), sc[i]};
        if (explain_before(prev, x) && explain_before(x, best)) best = x;
    }
    return explain_wave_first(best);
}

// what pass 2 and the final write make of one present max-mer; Sw, Sg: the row's exact sums
struct ExplainTerm {
    double pw, pg, term;
};
template <typename COUNT>
__device__ inline ExplainTerm explain_term(uint32_t code, int kmin, int kmax, const double* r, const double* __restrict__ ig, COUNT&& count,
                                           double Sw, double Sg) {
    const double LN2 = 0.69314718055994530942;
    unsigned long long W;
    double A;
    range_maxmer_window(code, kmin, kmax, r, count, W, A);
    const double Ig = ig[code];
    const double ratio = div_exact(A, double(W) * Ig);                  // as range_maxmer_add
    const double Iw = ratio * Ig;
    ExplainTerm t;
    t.pw = div_exact(Iw, Sw);
    t.pg = div_exact(Ig, Sg);
    t.term = t.pw * (log_pos(div_exact(t.pw, t.pg)) / LN2);
    return t;
}

// LDS of the selection: the waves' candidates of a round (two buffers), the winners' codes
template <int NW>
struct ExplainLds {
    unsigned long long key[2][NW];
    uint32_t code[2][NW];
    uint32_t win[FRISK_EXPLAIN_MAX];
};

// one wave's present max-mers of a step go behind the slice's entries; every lane of the wave calls (tl7: the slice's counter)
__device__ inline void explain_push(bool present, uint32_t code, uint32_t* tl7, uint32_t* sc, int64_t cap) {
    const unsigned long long m = __ballot(present);
    if (m == 0ull) return;                                              // (wave-uniform)
    const uint32_t before = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
    uint32_t base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(tl7, uint32_t(__popcll(m)));
    base = __builtin_amdgcn_readfirstlane(base);
    const int64_t at = int64_t(base) + before;
    if (present && at < cap) sc[at] = code;
}

// Pass 2, selection and write of one plainly kept row, every thread of the workgroup.  The slice holds the codes of the row's m
// entries; term_of(code): explain_term on the row's tables; count_top(code): the max-mer's own count.  Ends behind a barrier: the
// tables, the slice and the LDS may be rewritten.
template <int NT, typename TERM, typename COUNT>
__device__ inline void explain_select(const ExplainParams& E, int64_t row, uint32_t m, double* st, const uint32_t* sc,
                                      ExplainLds<NT / 64>& X, TERM&& term_of, COUNT&& count_top) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x;
    const uint32_t rounds = m < uint32_t(E.top_n) ? m : uint32_t(E.top_n);      // scalar: m is
    ExplainPick mine = explain_none();
    for (uint32_t i = tid; i < m; i += NT) {                                    // thread t scores entries t, t + NT, ...: its share
        const uint32_t code = sc[i];
        const double term = term_of(code).term;
        st[i] = term;
        const ExplainPick x = {explain_key(term), code};
        if (explain_before(x, mine)) mine = x;
    }
    for (uint32_t j = 0; j < rounds; ++j) {
        const ExplainPick w = explain_wave_first(mine);
        if ((tid & 63) == 0) { X.key[j & 1][tid >> 6] = w.key; X.code[j & 1][tid >> 6] = w.code; }
        __syncthreads();
        ExplainPick g = {X.key[j & 1][0], X.code[j & 1][0]};
#pragma unroll
        for (int v = 1; v < NW; ++v) {
            const ExplainPick y = {X.key[j & 1][v], X.code[j & 1][v]};
            if (explain_before(y, g)) g = y;
        }
        if (tid == 0) X.win[j] = g.code;
        // every other thread's candidate ranks behind g and stays the first of its share there; the owner's wave finds its next
        const unsigned long long own = __ballot(mine.code == g.code);       // (codes are distinct: at most one lane of the workgroup)
        if (own != 0ull) {                                                  // (wave-uniform)
            const int lane = __ffsll(own) - 1;
            const ExplainPick next = explain_share_next<NT>(st, sc, m, uint32_t((tid & ~63) + lane), g);
            if ((tid & 63) == lane) mine = next;
        }
    }
    __syncthreads();
    if (uint32_t(tid) < rounds) {
        const uint32_t code = X.win[tid];
        const ExplainTerm t = term_of(code);
        const int64_t at = row * E.top_n + tid;
        E.code[at] = code;
        E.count[at] = count_top(code);
        E.pw[at] = t.pw; E.pg[at] = t.pg; E.term[at] = t.term;
    }
    __syncthreads();
}

// the row's status as range_finish wrote it
__device__ inline uint32_t explain_status(uint32_t status, uint32_t nvalid_top, double Sg) {
    if (nvalid_top > 0 && Sg != Sg) status |= ROW_ZERO_WEIGHT;
    return status;
}

// ---- the mode ---------------------------------------------------------------------------------------------------------------
// walk, pass 1, range_finish and the selection of one row whose tables are ready (a mode of range_row_loop), on either form
template <int NW>
struct ExplainMode {
    const ExplainParams& E;
    double* red;                // NW * 6 doubles of LDS
    ExplainLds<NW>& X;
    double* st;                 // the workgroup's slice: terms ...
    uint32_t* sc;               // ... then codes
    __device__ ExplainMode(const ExplainParams& E_, double* red_, ExplainLds<NW>& X_)
        : E(E_), red(red_), X(X_), st(E_.stage + int64_t(blockIdx.x) * (E_.cap + E_.cap / 2)), sc(reinterpret_cast<uint32_t*>(st + E_.cap)) {}
    __device__ void dropped(int64_t) const {}
    template <typename FORM>
    __device__ void score(const FORM& form, int64_t row, uint32_t status0, uint32_t nvalid_top, const double* r) const {
        constexpr int NT = FORM::NT;
        static_assert(NT == NW * 64, "the form's workgroup");
        const RangeParams& P = E.R;
        const int kmin = form.kmin, kmax = form.kmax();
        uint32_t* tl7 = form.tl + 7;                                        // entries of the slice (cleared by form.tables)
        auto count = [&](int x, uint32_t c) -> uint32_t { return form.count(x, c); };

        // ---- walk: the present codes
        form.walk([&](bool present, uint32_t code) { explain_push(present, code, tl7, sc, E.cap); });
        __threadfence();
        __syncthreads();
        const int64_t staged = int64_t(range_uni(*tl7));
        const uint32_t m = uint32_t(staged < E.cap ? staged : E.cap);

        // ---- pass 1: PlainMode's stages 3 + 4
        ExactSum accw = exact_begin(), accg = exact_begin(), acct = exact_begin();
        for (uint32_t i = threadIdx.x; i < m; i += NT) range_score_maxmer(sc[i], kmin, kmax, r, P.ig, count, accw, accg, acct);
        range_finish<NW>(P, row, status0, nvalid_top, accw, accg, acct, red);   // (its barrier: pass 1 has read the tables)
        const double Sw = exact_value(accw), Sg = exact_value(accg);
        if (threadIdx.x == 0) E.n_present[row] = int32_t(m);
        if (range_uni(explain_status(status0, nvalid_top, Sg)) == ROW_KEPT)
            explain_select<NT>(E, row, m, st, sc, X,
                               [&](uint32_t code) { return explain_term(code, kmin, kmax, r, P.ig, count, Sw, Sg); },
                               [&](uint32_t code) { return count(kmax, code); });
    }
};

template <bool K8>
__global__ __launch_bounds__(FRISK_RANGE_NT) void explain_short_kernel(const ExplainParams E) {
    constexpr int NW = FRISK_RANGE_NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint32_t tl[8];
    __shared__ double red[NW * 6];
    __shared__ ExplainLds<NW> X;
    ShortForm<K8> form(E.R, lds, tl);
    range_row_loop(E.R, form, ExplainMode<NW>(E, red, X));
}

__global__ __launch_bounds__(FRISK_RANGE_BIG_NT) void explain_long_kernel(const ExplainParams E, uint32_t* __restrict__ big, int64_t big_stride) {
    constexpr int NW = FRISK_RANGE_BIG_NT / 64;
    __shared__ uint32_t tl[8];
    __shared__ double red[NW * 6];
    __shared__ ExplainLds<NW> X;
    LongForm form(E.R, big, big_stride, tl);
    range_row_loop(E.R, form, ExplainMode<NW>(E, red, X));
}
