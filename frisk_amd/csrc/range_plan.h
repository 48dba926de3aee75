// range_plan.h - everything the host decides about one call of the region scorer (frisk_ranges.hip) before it touches the device,
// as a plain value computed by a pure function: the row checks, the (resident position, length) pairs, the two lists longest first,
// the hand-over capacity, the slice capacities of frisk_explain_ranges, the short form's grid and the long form's wanted workgroups,
// and the fit of those workgroups into free memory.  No HIP here: frisk_ranges.hip fills the arguments from the context and walks
// the plan; tools/exp/san_host.cpp computes and checks plans on a CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/frisk_hip.h"      // FRISK_E_* (found without an include path of its own)

#define FRISK_RANGE_SHORT_MAX 65535 // longest range of the short form (16-bit counters)
#define FRISK_RANGE_HANDOVER_WGS 8  // long form: workgroups launched for the rows the short form may hand over

struct RangePlan {
    int error_code = FRISK_OK;          // != FRISK_OK: `error` is the message behind "<entry point>: ", nothing else is set
    std::string error;
    std::vector<int64_t> ranges;        // per caller's row: resident position of the first base, length
    std::vector<int64_t> short_rows, long_rows;     // the rows of each form, longest first (ties by row: a function of the call alone)
    int64_t long_cap = 0;               // entries of the long form's list: its own rows and every row the short form may hand over
    int64_t cap_short = 0, cap_long = 0;    // explain: entries of a workgroup's slice per form (0 without top_n)
    int grid_short = 0;                 // workgroups of the short form
    int64_t want_long = 0;              // ... of the long form, before the memory fit
    int64_t n_short() const { return int64_t(short_rows.size()); }
    int64_t n_long() const { return int64_t(long_rows.size()); }
};

// seq_index / start / stop: the caller's n rows; n_seq, seq_len, seq_off: the resident batch.  all_long: every row to the long form
// (kmax > 8, FRISK_RANGES_BIG).  per_cu_short: workgroups of the short form a CU holds beside each other when kmax < 8 (at
// kmax = 8 the order-8 table leaves room for one).  top_n: frisk_explain_ranges' (0: the slices are not planned).
inline RangePlan plan_ranges(int32_t n_seq, const int64_t* seq_len, const int64_t* seq_off, const int32_t* seq_index, const int64_t* start,
                             const int64_t* stop, int64_t n, int kmax, bool all_long, int num_cu, int per_cu_short, int top_n) {
    RangePlan R;
    auto refuse = [&](const char* what, int64_t row) {
        R = RangePlan();
        R.error_code = FRISK_E_ARG;
        R.error = std::string(what) + " in row " + std::to_string(row);
        return R;
    };
    R.ranges.resize(size_t(n) * 2);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t s = seq_index[r];
        if (s < 0 || s >= n_seq) return refuse("sequence index out of range", r);
        if (start[r] < 0 || stop[r] <= start[r] || stop[r] > seq_len[size_t(s)] || stop[r] - start[r] > int64_t(0x7FFFFFFF))
            return refuse("range outside the scaffold (or empty, or of 2^31 bases or more)", r);
        R.ranges[size_t(2 * r)] = seq_off[size_t(s)] + start[r];
        R.ranges[size_t(2 * r + 1)] = stop[r] - start[r];
    }
    auto len = [&](int64_t r) { return R.ranges[size_t(2 * r + 1)]; };
    std::vector<int64_t> order(static_cast<size_t>(n));
    std::iota(order.begin(), order.end(), int64_t(0));
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return len(a) != len(b) ? len(a) > len(b) : a < b; });
    for (int64_t r : order) (all_long || len(r) > FRISK_RANGE_SHORT_MAX ? R.long_rows : R.short_rows).push_back(r);
    const bool k8 = kmax == 8;
    const int64_t n_short = R.n_short(), n_long = R.n_long();
    R.long_cap = n_long + (k8 ? n_short : 0);           // every short row of kmax = 8 may be handed over
    if (top_n > 0) {
        // a range of len bases has at most min(len, 4^kmax) distinct max-mers (even: the 32-bit codes lie behind the terms)
        auto slice_cap = [&](int64_t longest) { return (std::min<int64_t>(longest, int64_t(1) << (2 * kmax)) + 1) / 2 * 2; };
        const int64_t len_short = n_short ? len(R.short_rows[0]) : 0, len_long = n_long ? len(R.long_rows[0]) : 0;
        R.cap_short = slice_cap(len_short);
        R.cap_long = slice_cap(std::max(len_long, k8 ? len_short : 0));
    }
    R.grid_short = int(std::min<int64_t>(n_short, int64_t(num_cu) * (kmax == 8 ? 1 : per_cu_short)));
    // The short rows of kmax = 8 may all be handed over, but hardly any is: they add a few workgroups to the grid, not one each
    // (the grid-stride loop takes whatever the list holds in the end).
    R.want_long = std::min<int64_t>(n_long + std::min<int64_t>(R.long_cap - n_long, FRISK_RANGE_HANDOVER_WGS), num_cu);
    return R;
}

// ---- frisk_refine_ranges ----------------------------------------------------------------------------------------------------
#define FRISK_REFINE_MAX_FLANK 65536
#define FRISK_REFINE_GEOM 6         // entries of a row's geometry

// why a call's flank or order is refused (nullptr: they are fine); the chain of order r reads the counts of order r + 1
inline const char* refine_args_problem(int32_t flank, int32_t order, int kmin, int kmax) {
    if (flank < 1 || flank > FRISK_REFINE_MAX_FLANK) return "flank outside 1 .. 65536";
    if (order < 0 || order + 1 < kmin || order + 1 > kmax) return "the chain of order r reads the counts of order r + 1, which must lie in kmin .. kmax";
    return nullptr;
}

// The plan of the CORES [a + Fe, b - Fe), Fe = min(flank, (b - a) / 4), as plan_ranges plans any rows, and per caller's row the
// geometry of the search: resident position of the scaffold's first base, a, b, Fe, the bases searched left of a (the flank
// clipped at the scaffold's first base) and right of b (clipped at its last).  A region of fewer than four bases has Fe = 0: its
// core is the region itself - it takes a workgroup for its status and nn, which only the device can tell - and nothing is searched.
struct RefinePlan {
    RangePlan plan;                 // error_code / error: a refused call, nothing else is set
    std::vector<int64_t> geom;      // FRISK_REFINE_GEOM per caller's row
};
inline RefinePlan plan_refine(int32_t n_seq, const int64_t* seq_len, const int64_t* seq_off, const int32_t* seq_index, const int64_t* start,
                              const int64_t* stop, int64_t n, int32_t flank, int32_t order, int kmin, int kmax, bool all_long, int num_cu,
                              int per_cu_short) {
    RefinePlan R;
    auto refuse = [&](const std::string& what) {
        R = RefinePlan();
        R.plan.error_code = FRISK_E_ARG;
        R.plan.error = what;
        return R;
    };
    if (const char* bad = refine_args_problem(flank, order, kmin, kmax)) return refuse(bad);
    std::vector<int64_t> core_start(static_cast<size_t>(n)), core_stop(static_cast<size_t>(n));
    R.geom.resize(size_t(n) * FRISK_REFINE_GEOM);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t s = seq_index[r];
        if (s < 0 || s >= n_seq) return refuse("sequence index out of range in row " + std::to_string(r));
        const int64_t a = start[r], b = stop[r], L = seq_len[size_t(s)];
        if (a < 0 || b <= a || b > L || b - a > int64_t(0x7FFFFFFF))
            return refuse("range outside the scaffold (or empty, or of 2^31 bases or more) in row " + std::to_string(r));
        const int64_t fe = std::min<int64_t>(flank, (b - a) / 4);
        core_start[size_t(r)] = a + fe;
        core_stop[size_t(r)] = b - fe;
        int64_t* g = R.geom.data() + size_t(r) * FRISK_REFINE_GEOM;
        g[0] = seq_off[size_t(s)]; g[1] = a; g[2] = b; g[3] = fe;
        g[4] = std::min(fe, a);
        g[5] = std::min(fe, L - b);
    }
    R.plan = plan_ranges(n_seq, seq_len, seq_off, seq_index, core_start.data(), core_stop.data(), n, kmax, all_long, num_cu, per_cu_short, 0);
    if (R.plan.error_code) R.geom.clear();
    return R;
}

// The long form's workgroups that fit: each takes `stride` 32-bit words of tables and slice_bytes more (explain); half of the
// free memory may go to them, beside what the table buffer (have_words) holds already.  The device is asked for free_bytes only
// when the buffer is too small for `want` or a slice is needed; this is what is made of the answer.
inline int64_t fit_long_workgroups(int64_t want, int64_t stride, size_t slice_bytes, size_t free_bytes, size_t have_words) {
    const int64_t fit = int64_t((free_bytes / 2 + have_words * 4) / (size_t(stride) * 4 + slice_bytes));
    return std::max<int64_t>(1, std::min(want, fit));
}
