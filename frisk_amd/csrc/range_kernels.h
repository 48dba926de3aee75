// range_kernels.h - frisk_score_ranges: one iteration of the reference's scan loop (L1478-1494: computeKmers(window) L280-367, both
// IvomBuilds L369-457, KLD L459-472, calcGC L120-137, calcRIP L474-495) on ARBITRARY ranges of the resident batch, one workgroup
// per range.  A range is scored as the slice it is: no word reaches past its last base, whatever follows it in the scaffold.
//
// Geometry comes from a device array of (resident position, length) pairs indexed by the caller's row; the rows themselves are
// handed out longest first (the host sorts the index, the workgroups take it by grid stride), and results are written at the
// caller's row.  Two forms share one scoring body - scan_big_kernel.h's: every non-empty bin of the order-K table is a present
// max-mer (no election), closed-form IVOM, one-pass KLD, ExactSum - so a row's bits depend on the range and the profile alone,
// not on the form, the grid or the order of the rows:
//
//   short  kmax <= 8, length <= 65 535: every table is a 16-bit counter in LDS (a count cannot exceed the length).  kmax <= 7 holds
//          the orders kmin..kmax directly (43.7 KB at 1..7: three workgroups per CU).  kmax = 8: order 8 takes 128 KiB; the orders
//          kmin..6 get one update at min(run, 6) and are marginalised downwards in LDS; order 7 is the sum of the four order-8
//          children plus an orphan list (WinTables<true>::count) - orders 1..7 stored outright would need 171 KB beside nothing
//          and a CU has 160.  Two orphans lie at least 8 positions apart, so a range of n bases holds at most floor((n - 7) / 8) + 1
//          of them; a list lookup is linear, hence the list is capped at FRISK_RANGE_ORPHANS entries and a range that overflows
//          the cap is appended to a device list that the long form scores in the same call.  Tables are cleared per range.
//   long   kmax >= 9, length > 65 535, handed-over ranges, FRISK_RANGES_BIG: 32-bit tables of all orders in a per-workgroup slice
//          of global scratch, with scan_big_kernel.h's fences around the atomics and its zeroing behind each range.
//
// A FORM hides the table format (ShortForm<K8>, LongForm: NT, tables, count, walk, release).  A MODE is what is done with a row
// whose tables are ready: PlainMode here scores inside the walk (at K = 8 in a loop of its own, see there); panel_kernels.h and
// explain_kernels.h bring theirs, refine_kernels.h one that does not score at all.  The row loop (range_row_loop) is written once for every form and mode; a __global__ entry
// point declares its LDS, makes a form and a mode and runs the loop.
//
// FP64 throughout, no MFMA, no floating-point atomics.
#pragma once
#include "scan_kernel.h"
#include "range_plan.h"     // FRISK_RANGE_SHORT_MAX, FRISK_RANGE_HANDOVER_WGS: what the host decides

#pragma clang fp contract(off)

#define FRISK_RANGE_NT 512          // short form: threads per workgroup
#define FRISK_RANGE_BIG_NT 1024     // long form
#define FRISK_RANGE_ORPHANS 64      // short form, kmax = 8: entries of the orphan list in LDS

struct RangeParams {
    const uint32_t* codes;
    const uint32_t* inv;
    const uint32_t* low;
    const double* ig;           // genome-side IVOM, 4^kmax entries (NaN = zero weight)
    const int64_t* ranges;      // per caller's row: resident position of the first base, length
    const int64_t* list;        // the rows of this launch, longest first
    int64_t n_list;             // ... as many as the host put there
    const unsigned int* more;   // long form: behind them, *more rows that the short form appended (nullptr: none)
    int64_t* out_list;          // short form, kmax = 8: rows whose orphan list overflowed are appended here ...
    unsigned int* out_count;    // ... and counted
    int32_t kmin, kmax;
    uint32_t rip;               // != 0: fill pi / si / cri
    // outputs, indexed by the caller's row
    uint32_t* status;
    double* kld;
    double* gc;
    double* pi;
    double* si;
    double* cri;
    int64_t* nn;
};

// LDS of the short form: [order-8 table] [small tables, u16 bins] [orphan list]; every part a multiple of 16 bytes
struct RangeLds {
    uint32_t t8_bytes, small, small_bytes, orphans, total;
};
__host__ __device__ inline RangeLds range_lds(int kmin, int kmax) {
    RangeLds L;
    const bool k8 = kmax == 8;
    const int ks = k8 ? 6 : kmax;
    L.t8_bytes = k8 ? FRISK_T8_BYTES : 0;
    L.small = L.t8_bytes;
    const int64_t bins = ks >= kmin ? table_offset(kmin, ks + 1) : 0;
    L.small_bytes = uint32_t((bins * 2 + 15) / 16 * 16);
    L.orphans = L.small + L.small_bytes;
    L.total = L.orphans + (k8 ? FRISK_RANGE_ORPHANS * 2 : 0);
    if (L.total < 16) L.total = 16;
    return L;
}

// A workgroup-uniform value read back from LDS, moved to a scalar register: every branch on it - a range handed over or left
// unscored - is then a scalar branch, as in scan_kernel.h.
__device__ inline uint32_t range_uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// Rows are dealt by grid stride over the launch's list (longest first, so a workgroup's k-th row is among the k-th longest
// gridDim.x).  The loop's bounds must stay scalar - a kernel argument and one scalar load - as every branch around its barriers.
__device__ inline int64_t range_rows(const RangeParams& P) {
    return P.n_list + (P.more != nullptr ? int64_t(*P.more) : 0);      // the rows the short form appended follow the host's
}

// a range that the N filter drops (L238): no FRISK_ROW_KEPT, NaN in every double column
__device__ inline void range_write_unresolved(const RangeParams& P, int64_t row, int64_t nn) {
    const double qnan = __longlong_as_double(0x7FF8000000000000LL);
    P.status[row] = 0u;
    P.nn[row] = nn;
    P.kld[row] = qnan; P.gc[row] = qnan;
    if (P.rip) { P.pi[row] = qnan; P.si[row] = qnan; P.cri[row] = qnan; }
}

// composition, RIP indices (calcRIP L474-495; codes: AT=1 TA=4 TG=6 GT=9 CA=12 AC=3) and nn of a kept row; one thread
template <typename COUNT>
__device__ inline void range_write_composition(const RangeParams& P, int64_t row, int64_t S, int64_t gcount, int64_t nn, COUNT&& count) {
    P.nn[row] = nn;
    P.gc[row] = double(gcount) / double(S);                             // L136
    if (P.rip) {
        const double qnan = __longlong_as_double(0x7FF8000000000000LL);
        const uint32_t AT = count(2, 1u), TA = count(2, 4u), TG = count(2, 6u), GT = count(2, 9u), CA = count(2, 12u), AC = count(2, 3u);
        const double pi = AT > 0 ? double(TA) / double(AT) : qnan;
        const double si = (AC + GT) > 0 ? double(CA + TG) / double(AC + GT) : qnan;
        P.pi[row] = pi;
        P.si[row] = si;
        P.cri[row] = (pi == 0.0 || si == 0.0) ? qnan : pi - si;         // "if PI and SI" (L491): 0.0 is falsy
    }
}

// window constants r_x = 4^x / D_x, D_x = (S - (x - 1)) * 2 (L401-409)
__device__ inline void range_constants(int64_t S, double* r) {
    for (int x = 0; x <= FRISK_MAX_K; ++x) r[x] = double(1u << (2 * x)) / double((S - (x - 1)) * 2);
}

// THE scoring body: one present max-mer - window-side IVOM in closed form from the counts of its prefixes, genome side from the
// table, three exact additions.  count(x, c): occurrences of the x-mer c in the range.  In two halves: what the range alone
// decides (W, A), and what a profile's value Ig adds to its three sums - panel_kernels.h runs the second once per profile.
template <typename COUNT>
__device__ inline void range_maxmer_window(uint32_t code, int kmin, int kmax, const double* r, COUNT&& count, unsigned long long& W,
                                           double& A) {
    W = 0;
    A = 0.0;
#pragma unroll
    for (int x = 1; x <= FRISK_MAX_K; ++x) {
        if (x < kmin || x > kmax) continue;
        const uint32_t cx = count(x, code >> (2 * (kmax - x)));
        const double cd = double(cx);
        W += (unsigned long long)cx << (2 * x);                         // count * 4**x (L399-408)
        A = __builtin_fma(cd * cd, r[x], A);                            // w_x * p_x = c^2 4^x / D_x
    }
}
__device__ inline void range_maxmer_add(double A, double Wd, double Ig, ExactSum& accw, ExactSum& accg, ExactSum& acct) {
    const double ratio = div_exact(A, Wd * Ig);
    const double Iw = ratio * Ig;
    exact_add(accw, Iw);
    exact_add(accg, Ig);
    exact_add(acct, Iw * log_pos(ratio));
}
template <typename COUNT>
__device__ inline void range_score_maxmer(uint32_t code, int kmin, int kmax, const double* r, const double* __restrict__ ig,
                                          COUNT&& count, ExactSum& accw, ExactSum& accg, ExactSum& acct) {
    unsigned long long W;
    double A;
    range_maxmer_window(code, kmin, kmax, r, count, W, A);
    range_maxmer_add(A, double(W), ig[code], accw, accg, acct);
}

// the three sums over the workgroup, the KLD (L453-454, L465-470) and the row's status; every thread calls, thread 0 writes
template <int NW>
__device__ inline void range_finish(const RangeParams& P, int64_t row, uint32_t status, uint32_t nvalid_top, ExactSum& accw,
                                    ExactSum& accg, ExactSum& acct, double* red) {
    exact_end(accw); exact_end(accg); exact_end(acct);
    block_sum3<NW>(accw, accg, acct, red, int(threadIdx.x));
    const double Sw = exact_value(accw), Sg = exact_value(accg), Tt = exact_value(acct);
    const double LN2 = 0.69314718055994530942;
    double acc = (nvalid_top == 0) ? 0.0 : ((Tt / Sw - log(Sw)) + log(Sg)) / LN2;
    if (nvalid_top > 0 && Sg != Sg) status |= ROW_ZERO_WEIGHT;          // a max-mer without genome weight (L437)
    if (status & ROW_ZERO_WEIGHT) acc = __longlong_as_double(0x7FF8000000000000LL);
    if (threadIdx.x == 0) {
        P.status[row] = status;
        P.kld[row] = acc;
    }
}

// status bits of a kept row known before scoring
__device__ inline uint32_t range_status(uint32_t nvalid_top, int64_t S, int kmin, int kmax) {
    uint32_t status = ROW_KEPT;
    if (nvalid_top == 0) status |= ROW_NO_MAXMER;
    if (nvalid_top > 0 && S >= kmin - 1 && S <= kmax - 1) status |= ROW_ZERO_WEIGHT;        // a zero divisor D_x (L401-409)
    return status;
}

// what stages 1 and 2 make of a row (workgroup-uniform): its tables are ready to be scored, the long form takes it over, or the
// N rule drops it
enum { RANGE_ROW_SCORE = 0, RANGE_ROW_HANDED = 1, RANGE_ROW_DROPPED = 2 };

struct NoStep { __device__ void operator()() const {} };     // walk(f) without a per-step hook

// ---- short form -------------------------------------------------------------------------------------------------------------
template <bool K8>
struct ShortForm {
    static constexpr int NT = FRISK_RANGE_NT;
    unsigned char* lds;         // range_lds(kmin, kmax)
    uint32_t* tl;               // 8 words of LDS: [0..5] the row's counters, [7] the mode's
    int kmin, kmax_;
    WinTables<K8> T;

    __device__ ShortForm(const RangeParams& P, unsigned char* lds_, uint32_t* tl_) : lds(lds_), tl(tl_), kmin(P.kmin), kmax_(P.kmax) {}
    __device__ int kmax() const { return K8 ? 8 : kmax_; }
    // occurrences of the x-mer c in the row
    __device__ uint32_t count(int x, uint32_t c) const { return T.count(x, c); }

    // Stages 1 and 2 of one row, every thread of the workgroup: clear, count, composition, the N rule, marginalisation; gc / RIP /
    // nn of a kept row and every column of a dropped one are written here.  Ends behind a barrier: the tables may be read.
    __device__ int tables(const RangeParams& P, int64_t row, int64_t& S, uint32_t& nvalid_top) {
        const int tid = threadIdx.x, lane = tid & 63;
        // the last row's view ends here: carried round the row loop it keeps scalar registers live through stage 1, and the
        // scoring bodies then read spilled ones back (1 % of the short kernels' time, measured)
        T = WinTables<K8>();
        const int kmax = this->kmax();
        const int ks = K8 ? 6 : kmax;                       // highest order kept in the small tables
        const RangeLds L = range_lds(kmin, kmax);
        uint32_t* t8 = reinterpret_cast<uint32_t*>(lds);
        uint32_t* small32 = reinterpret_cast<uint32_t*>(lds + L.small);
        uint16_t* small16 = reinterpret_cast<uint16_t*>(lds + L.small);
        uint16_t* orph = reinterpret_cast<uint16_t*>(lds + L.orphans);
        const int64_t g0 = P.ranges[2 * row];
        const int n = int(P.ranges[2 * row + 1]);       // <= FRISK_RANGE_SHORT_MAX
        // ---- clear: 128 KiB over 512 threads is 16 uint4 stores each
        if (K8) for (int i = tid; i < int(L.t8_bytes / 16); i += NT) reinterpret_cast<uint4*>(t8)[i] = make_uint4(0, 0, 0, 0);
        for (uint32_t i = tid; i < L.small_bytes / 16; i += NT) reinterpret_cast<uint4*>(small32)[i] = make_uint4(0, 0, 0, 0);
        if (tid < 8) tl[tid] = 0;
        __syncthreads();

        // ---- stage 1: one small-table update per position at the order of its longest valid word (<= 6 at K = 8), the order-8
        // update or the orphan list; uppercase composition by wave ballots
        uint32_t cA = 0, cT = 0, cG = 0, cC = 0, ntop = 0;
        for (int base = 0; base < n; base += NT) {
            const int jj = base + tid;
            const bool act = jj < n;
            const int64_t g = g0 + (act ? jj : 0);                          // clamped: loads are unconditional
            const uint32_t c16 = fetch_codes16(P.codes, g);
            const uint32_t inv8 = fetch_mask8(P.inv, g);
            const uint32_t low1 = fetch_mask1(P.low, g);
            int run = lead_clear8(inv8);                                    // window words are upper-cased: L334-335
            const int rem = n - jj;
            run = run < rem ? run : rem;
            run = run < kmax ? run : kmax;
            if (act) {
                const int rs = run < ks ? run : ks;
                if (rs >= kmin) {
                    const uint32_t b = uint32_t(table_offset(kmin, rs)) + (c16 >> (16 - 2 * rs));
                    atomicAdd(&small32[b >> 1], 1u << ((b & 1u) * 16));
                }
                if (K8) {
                    if (run == 8) atomicAdd(&t8[c16 >> 1], 1u << ((c16 & 1u) * 16));
                    else if (run == 7 && kmin <= 7) {
                        const uint32_t slot = atomicAdd(&tl[5], 1u);
                        if (slot < FRISK_RANGE_ORPHANS) orph[slot] = uint16_t(c16 >> 2);
                    }
                }
            }
            const bool up = act && !((inv8 >> 7) | low1);
            const uint32_t c2 = c16 >> 14;
            cA += __popcll(__ballot(up && c2 == 0));
            cT += __popcll(__ballot(up && c2 == 1));
            cG += __popcll(__ballot(up && c2 == 2));
            cC += __popcll(__ballot(up && c2 == 3));
            ntop += __popcll(__ballot(act && run == kmax));
        }
        if (lane == 0) {
            if (cA) atomicAdd(&tl[0], cA);
            if (cT) atomicAdd(&tl[1], cT);
            if (cG) atomicAdd(&tl[2], cG);
            if (cC) atomicAdd(&tl[3], cC);
            if (ntop) atomicAdd(&tl[4], ntop);
        }
        __syncthreads();
        const int64_t upA = range_uni(tl[0]), upT = range_uni(tl[1]), upG = range_uni(tl[2]), upC = range_uni(tl[3]);
        nvalid_top = range_uni(tl[4]);
        const int n_orph = K8 ? int(range_uni(tl[5])) : 0;
        if (K8 && n_orph > FRISK_RANGE_ORPHANS) {       // the list is incomplete: the long form scores this row
            if (tid == 0) P.out_list[atomicAdd(P.out_count, 1u)] = row;
            __syncthreads();                            // the counters are cleared for the next range only after every read of them
            return RANGE_ROW_HANDED;
        }
        S = upA + upT + upG + upC;                                          // windowSpace (L380)
        const int64_t nn = int64_t(n) - S;
        if (double(nn) >= 0.3 * double(n)) {                                // L237-241 / L213, in double like CPython
            if (tid == 0) range_write_unresolved(P, row, nn);
            __syncthreads();
            return RANGE_ROW_DROPPED;
        }

        // ---- stage 2: marginalise the small tables: C_x[q] = D_x[q] + sum_b C_{x+1}[4q+b]
        for (int x = ks - 1; x >= kmin; --x) {
            const uint32_t ox = uint32_t(table_offset(kmin, x)), ou = uint32_t(table_offset(kmin, x + 1));
            for (uint32_t c = tid; c < (1u << (2 * x)); c += NT) {
                const uint2 ch = *reinterpret_cast<const uint2*>(small16 + ou + 4 * c);     // 8-byte aligned
                small16[ox + c] = uint16_t(small16[ox + c] + (ch.x & 0xFFFFu) + (ch.x >> 16) + (ch.y & 0xFFFFu) + (ch.y >> 16));
            }
            __syncthreads();
        }
        T.t8_16 = reinterpret_cast<const uint16_t*>(t8);
        T.small16 = small16;
        T.orph = orph; T.n_orph = n_orph;
        T.o0 = T.o1 = T.o2 = T.o3 = 0xFFFFFFFFu;
        if (K8) {
            if (n_orph > 0) T.o0 = orph[0];
            if (n_orph > 1) T.o1 = orph[1];
            if (n_orph > 2) T.o2 = orph[2];
            if (n_orph > 3) T.o3 = orph[3];
        }
        T.kmin = kmin;
        if (tid == 0) range_write_composition(P, row, S, upG + upC, nn, [&](int x, uint32_t c) { return count(x, c); });
        return RANGE_ROW_SCORE;
    }

    // f(present, code) for every bin of the order-K table, step() behind each step of the workgroup over it.  Every lane of a
    // wave is in every call of f; a step whose bins are empty in the whole wave is skipped (wave-uniform), step() with it.  No
    // workgroup barrier.
    template <typename F, typename STEP = NoStep>
    __device__ void walk(F&& f, STEP&& step = STEP()) const {
        const uint32_t tid = threadIdx.x;
        const uint32_t nK = 1u << (2 * kmax());
        if (K8) {
            const uint4* t8 = reinterpret_cast<const uint4*>(lds);
            for (uint32_t base = 0; base < nK / 8; base += NT) {            // eight bins per read; nK / 8 is a multiple of NT
                const uint32_t grp = base + tid;
                const uint4 v = t8[grp];
                if (__ballot((v.x | v.y | v.z | v.w) != 0u) == 0ull) continue;
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int b = 0; b < 8; ++b) f(((w[b >> 1] >> ((b & 1) * 16)) & 0xFFFFu) != 0u, 8 * grp + b);
                step();
            }
        } else {
            const uint16_t* top = T.small16 + uint32_t(table_offset(kmin, kmax()));
            for (uint32_t base = 0; base < nK; base += NT) {                // one bin per lane and step
                const uint32_t code = base + tid;
                f(code < nK && top[code < nK ? code : 0u] != 0, code);
                step();
            }
        }
    }

    // the tables are cleared at the head of the next row
    __device__ void release() const {}
};

// ---- long form --------------------------------------------------------------------------------------------------------------
// `big`: one slice of `big_stride` 32-bit words per workgroup, all-zero at launch and between ranges
// the slice is zeroed by ordinary stores, made visible at L2 before the next range's atomics
__device__ inline void range_zero_tables(uint32_t* cnt, int64_t big_stride) {
    for (int64_t i = threadIdx.x; i < big_stride / 4; i += FRISK_RANGE_BIG_NT) reinterpret_cast<uint4*>(cnt)[i] = make_uint4(0, 0, 0, 0);
    __threadfence();
}

struct LongForm {
    static constexpr int NT = FRISK_RANGE_BIG_NT;
    uint32_t* cnt;              // the workgroup's slice
    int64_t big_stride;
    uint32_t* tl;               // 8 words of LDS: [0..4] the row's counters, [7] the mode's
    int kmin, kmax_;

    __device__ LongForm(const RangeParams& P, uint32_t* big, int64_t big_stride_, uint32_t* tl_)
        : cnt(big + int64_t(blockIdx.x) * big_stride_), big_stride(big_stride_), tl(tl_), kmin(P.kmin), kmax_(P.kmax) {}
    __device__ int kmax() const { return kmax_; }
    __device__ uint32_t count(int x, uint32_t c) const { return cnt[table_offset(kmin, x) + c]; }

    // Stages 1 and 2 of one row on the workgroup's slice, as ShortForm::tables; a dropped row's slice is zeroed again here, a
    // scored row's by release() behind its last read.
    __device__ int tables(const RangeParams& P, int64_t row, int64_t& S, uint32_t& nvalid_top) {
        const int kmax = this->kmax();
        const int tid = threadIdx.x, lane = tid & 63;
        const int64_t g0 = P.ranges[2 * row], n = P.ranges[2 * row + 1];
        if (tid < 8) tl[tid] = 0;
        __syncthreads();

        // ---- stage 1: one global-atomic update per position; uppercase composition by wave ballots
        uint32_t cA = 0, cT = 0, cG = 0, cC = 0, ntop = 0;
        for (int64_t base = 0; base < n; base += NT) {
            const int64_t jj = base + tid;
            const bool act = jj < n;
            const int64_t g = g0 + (act ? jj : 0);
            const uint32_t c24 = fetch_codes24(P.codes, g);                 // 12 bases: orders up to FRISK_MAX_K
            const uint32_t inv16 = fetch_mask16(P.inv, g);
            const uint32_t low1 = fetch_mask1(P.low, g);
            int run = lead_clear16(inv16);
            const int64_t rem = n - jj;
            run = run < rem ? run : int(rem);
            run = run < kmax ? run : kmax;
            if (act && run >= kmin) atomicAdd(&cnt[table_offset(kmin, run) + (c24 >> (24 - 2 * run))], 1u);
            const bool up = act && !((inv16 >> 15) | low1);
            const uint32_t c2 = c24 >> 22;
            cA += __popcll(__ballot(up && c2 == 0));
            cT += __popcll(__ballot(up && c2 == 1));
            cG += __popcll(__ballot(up && c2 == 2));
            cC += __popcll(__ballot(up && c2 == 3));
            ntop += __popcll(__ballot(act && run == kmax));
        }
        if (lane == 0) {
            if (cA) atomicAdd(&tl[0], cA);
            if (cT) atomicAdd(&tl[1], cT);
            if (cG) atomicAdd(&tl[2], cG);
            if (cC) atomicAdd(&tl[3], cC);
            if (ntop) atomicAdd(&tl[4], ntop);
        }
        // the updates were made by atomics at L2; the tables are read with ordinary loads from here on: drop whatever this
        // CU's vector L1 still holds of them (agent-scope acquire = L1 invalidate), on both sides of the barrier
        __threadfence();
        __syncthreads();
        const int64_t upA = range_uni(tl[0]), upT = range_uni(tl[1]), upG = range_uni(tl[2]), upC = range_uni(tl[3]);
        nvalid_top = range_uni(tl[4]);
        S = upA + upT + upG + upC;
        const int64_t nn = n - S;
        if (double(nn) >= 0.3 * double(n)) {
            range_zero_tables(cnt, big_stride);
            if (tid == 0) range_write_unresolved(P, row, nn);
            __syncthreads();
            return RANGE_ROW_DROPPED;
        }
        // ---- stage 2: C_x[q] = D_x[q] + sum_b C_{x+1}[4q+b], level by level
        for (int x = kmax - 1; x >= kmin; --x) {
            const int64_t ox = table_offset(kmin, x), ou = table_offset(kmin, x + 1);
            for (uint32_t c = tid; c < (1u << (2 * x)); c += NT) {
                const uint4 ch = *reinterpret_cast<const uint4*>(cnt + ou + 4 * c);
                cnt[ox + c] += ch.x + ch.y + ch.z + ch.w;
            }
            __syncthreads();
        }
        if (tid == 0) range_write_composition(P, row, S, upG + upC, nn, [&](int x, uint32_t c) { return count(x, c); });
        return RANGE_ROW_SCORE;
    }

    // as ShortForm::walk, one bin per lane and step
    template <typename F, typename STEP = NoStep>
    __device__ void walk(F&& f, STEP&& step = STEP()) const {
        const uint32_t nK = 1u << (2 * kmax());
        const uint32_t* top = cnt + table_offset(kmin, kmax());
        for (uint32_t base = 0; base < nK; base += NT) {
            const uint32_t code = base + threadIdx.x;
            f(code < nK && top[code < nK ? code : 0u] != 0u, code);
            step();
        }
    }

    // behind a barrier: every read of the row's tables is done
    __device__ void release() const { range_zero_tables(cnt, big_stride); }
};

// ---- the row loop -----------------------------------------------------------------------------------------------------------
// Every row of the launch's list that falls to this workgroup: the form's tables, then the mode.  mode.dropped(row): a row the N
// rule drops, behind range_write_unresolved.  mode.score(form, row, status, nvalid_top, r): a row whose tables are ready; every
// thread calls, and it ends behind a barrier after its last read of the tables (range_finish's, or a later one) - release()
// follows.  Every branch here is on a workgroup-uniform scalar: the loop's bounds and what tables() returns.
template <typename FORM, typename MODE>
__device__ inline void range_row_loop(const RangeParams& P, FORM& form, MODE&& mode) {
    const int64_t n_rows = range_rows(P);
    for (int64_t q = blockIdx.x; q < n_rows; q += gridDim.x) {
        const int64_t row = P.list[q];
        int64_t S;
        uint32_t nvalid_top;
        const int what = form.tables(P, row, S, nvalid_top);
        if (what == RANGE_ROW_DROPPED) mode.dropped(row);
        if (what != RANGE_ROW_SCORE) continue;
        const uint32_t status = range_status(nvalid_top, S, form.kmin, form.kmax());
        double r[FRISK_MAX_K + 1];
        range_constants(S, r);
        mode.score(form, row, status, nvalid_top, r);
        form.release();
    }
}

// stages 3 + 4 of frisk_score_ranges: every non-empty bin of the order-K table is a present max-mer, scored inside the walk
struct PlainMode {
    const RangeParams& P;
    double* red;                // FORM::NT / 64 * 6 doubles of LDS
    __device__ void dropped(int64_t) const {}
    template <typename FORM>
    __device__ void score(const FORM& form, int64_t row, uint32_t status, uint32_t nvalid_top, const double* r) const {
        auto count = [&](int x, uint32_t c) -> uint32_t { return form.count(x, c); };
        ExactSum accw = exact_begin(), accg = exact_begin(), acct = exact_begin();
        if constexpr (std::is_same<FORM, ShortForm<true>>::value) {
            // Not through walk(), which is the same walk: with the scoring body handed to it as a lambda the K = 8 grid and
            // mixed workloads of tools/ranges_timing.py run 4 % longer (measured against this loop).  What the compiler is seen
            // to do differently there: a max-mer's six prefix-table addresses are formed in front of each of their loads, once
            // per bin, where this loop forms them once per group of eight.
            const uint4* t8 = reinterpret_cast<const uint4*>(form.lds);
            for (uint32_t grp = threadIdx.x; grp < (1u << 16) / 8; grp += FORM::NT) {       // eight bins per read
                const uint4 v = t8[grp];
                if ((v.x | v.y | v.z | v.w) == 0u) continue;
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    if (((w[b >> 1] >> ((b & 1) * 16)) & 0xFFFFu) == 0u) continue;
                    range_score_maxmer(8 * grp + b, form.kmin, 8, r, P.ig, count, accw, accg, acct);
                }
            }
        } else {
            form.walk([&](bool present, uint32_t code) {
                if (present) range_score_maxmer(code, form.kmin, form.kmax(), r, P.ig, count, accw, accg, acct);
            });
        }
        range_finish<FORM::NT / 64>(P, row, status, nvalid_top, accw, accg, acct, red);
    }
};

template <bool K8>
__global__ __launch_bounds__(FRISK_RANGE_NT) void range_short_kernel(const RangeParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint32_t tl[8];
    __shared__ double red[FRISK_RANGE_NT / 64 * 6];
    ShortForm<K8> form(P, lds, tl);
    range_row_loop(P, form, PlainMode{P, red});
}

__global__ __launch_bounds__(FRISK_RANGE_BIG_NT) void range_long_kernel(const RangeParams P, uint32_t* __restrict__ big, int64_t big_stride) {
    __shared__ uint32_t tl[8];
    __shared__ double red[FRISK_RANGE_BIG_NT / 64 * 6];
    LongForm form(P, big, big_stride, tl);
    range_row_loop(P, form, PlainMode{P, red});
}
