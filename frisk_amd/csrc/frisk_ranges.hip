// frisk_ranges.hip - frisk_score_ranges of the C ABI (include/frisk_hip.h): the scan loop's columns (KLD, GC, RIP indices) of
// arbitrary ranges of the resident batch against the context's finalised profile (range_kernels.h).  The host checks the rows,
// sorts them longest first (the workgroups of a launch take its list by grid stride), splits them between the two forms and
// queues both launches on the context's stream; a range the short form cannot hold reaches the long form through a device list,
// without a host round trip.  The context is frisk_ctx.h's; the scan's plan and row buffers are not touched.  gfx950 (MI355X)
// only.  frisk_score_ranges_panel and the panel's three calls are here too: the same host path with panel_kernels.h's kernels,
// every profile of the context's panel in one pass.  frisk_explain_ranges too: the same host path with explain_kernels.h's kernels,
// their scratch and the six arrays of the largest KLD terms.  Build: see __graft_entry__.build_hip().
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "frisk_ctx.h"
#include "range_kernels.h"
#include "panel_kernels.h"
#include "explain_kernels.h"

namespace {

template <bool K8>
hipError_t launch_short(const RangeParams& P, int grid, size_t lds, hipStream_t st) {
    auto kern = range_short_kernel<K8>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
    kern<<<grid, FRISK_RANGE_NT, lds, st>>>(P);
    return hipGetLastError();
}

template <bool K8>
hipError_t launch_panel_short(const PanelParams& Q, int grid, size_t lds, hipStream_t st) {
    auto kern = panel_short_kernel<K8>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
    kern<<<grid, FRISK_RANGE_NT, lds, st>>>(Q);
    return hipGetLastError();
}

template <bool K8>
hipError_t launch_explain_short(const ExplainParams& E, int grid, size_t lds, hipStream_t st) {
    auto kern = explain_short_kernel<K8>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
    kern<<<grid, FRISK_RANGE_NT, lds, st>>>(E);
    return hipGetLastError();
}

// frisk_explain_ranges' own arguments (host arrays)
struct ExplainOut {
    int32_t top_n;
    int32_t* n_present;
    uint32_t *code, *count;
    double *pw, *pg, *term;
};

// the three entry points: `panel` = score against the context's panel (np planes of status and kld) instead of its own profile;
// `ex` = the explain kernels and their outputs (never with `panel`)
int score_ranges(frisk_ctx* c, const bool panel, const ExplainOut* ex, const int32_t* seq_index, const int64_t* start, const int64_t* stop,
                 int64_t n, uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si, double* cri, int64_t* nn) {
    if (!c) return FRISK_E_ARG;
    const std::string who = ex ? "frisk_explain_ranges" : panel ? "frisk_score_ranges_panel" : "frisk_score_ranges";
    if (n < 0) return fail(c, FRISK_E_ARG, who + ": n < 0");
    if (ex && (ex->top_n < 1 || ex->top_n > FRISK_EXPLAIN_MAX)) return fail(c, FRISK_E_ARG, who + ": top_n outside 1 .. FRISK_EXPLAIN_MAX");
    const frisk_ctx::Batch& B = c->b();
    if (!B.have_seq) return fail(c, FRISK_E_ARG, who + ": no resident sequence batch");
    if (B.tiled) return fail(c, FRISK_E_ARG, who + ": the resident batch holds tiles, not whole scaffolds");
    const bool rip = (flags & FRISK_SCAN_RIP) != 0;
    if (rip && !(c->kmin <= 2 && c->kmax >= 2)) return fail(c, FRISK_E_ARG, "FRISK_SCAN_RIP needs kmin <= 2 <= kmax");
    if (panel ? c->panel_n == 0 : !c->profile_final) return fail(c, FRISK_E_STATE, who + (panel ? ": the panel is empty" : ": no finalised profile"));
    if (n == 0) return FRISK_OK;
    if (!seq_index || !start || !stop || !status || !kld || !gc || !nn || (rip && (!pi || !si || !cri)))
        return fail(c, FRISK_E_ARG, who + ": null array");
    if (ex && (!ex->n_present || !ex->code || !ex->count || !ex->pw || !ex->pg || !ex->term)) return fail(c, FRISK_E_ARG, who + ": null array");
    std::vector<int64_t> ranges(size_t(n) * 2);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t s = seq_index[r];
        if (s < 0 || s >= B.n_seq) return fail(c, FRISK_E_ARG, who + ": sequence index out of range in row " + std::to_string(r));
        if (start[r] < 0 || stop[r] <= start[r] || stop[r] > B.seq_len[size_t(s)] || stop[r] - start[r] > int64_t(0x7FFFFFFF))
            return fail(c, FRISK_E_ARG, who + ": range outside the scaffold (or empty, or of 2^31 bases or more) in row " + std::to_string(r));
        ranges[size_t(2 * r)] = B.seq_off[size_t(s)] + start[r];
        ranges[size_t(2 * r + 1)] = stop[r] - start[r];
    }
    // longest first (ties by row: the order is a function of the call alone), then one list per form
    std::vector<int64_t> order(static_cast<size_t>(n));
    std::iota(order.begin(), order.end(), int64_t(0));
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        const int64_t la = ranges[size_t(2 * a + 1)], lb = ranges[size_t(2 * b + 1)];
        return la != lb ? la > lb : a < b;
    });
    const bool k8 = c->kmax == 8;
    const bool all_long = (flags & FRISK_RANGES_BIG) != 0 || c->kmax > 8;
    std::vector<int64_t> short_rows, long_rows;
    for (int64_t r : order) (all_long || ranges[size_t(2 * r + 1)] > FRISK_RANGE_SHORT_MAX ? long_rows : short_rows).push_back(r);
    const int64_t n_short = int64_t(short_rows.size()), n_long = int64_t(long_rows.size());
    const int64_t long_cap = n_long + (k8 ? n_short : 0);       // every short row of kmax = 8 may be handed over
    // explain: entries of a workgroup's slice per form - a range of len bases has at most min(len, 4^kmax) distinct max-mers (even:
    // the 32-bit codes lie behind the terms)
    auto slice_cap = [&](int64_t longest) { return (std::min<int64_t>(longest, int64_t(1) << (2 * c->kmax)) + 1) / 2 * 2; };
    const int64_t len_short = n_short ? ranges[size_t(2 * short_rows[0] + 1)] : 0, len_long = n_long ? ranges[size_t(2 * long_rows[0] + 1)] : 0;
    const int64_t cap_short = slice_cap(len_short), cap_long = slice_cap(std::max(len_long, k8 ? len_short : 0));

    HIPC(c, hipSetDevice(c->device));
    if (int rc = settle_stream(c)) return rc;
    const size_t N = size_t(n);
    const size_t np = panel ? size_t(c->panel_n) : 1;            // planes of status and kld
    const int ncol = rip ? 4 : 1;                               // gc [pi si cri], behind the planes of kld
    DevBuf<int64_t> d_ranges, d_short, d_long, d_nn;            // (freed on every return below)
    DevBuf<unsigned int> d_cnt;                                 // [0]: rows handed over to the long form
    DevBuf<uint32_t> d_status;
    DevBuf<double> d_val, d_stage, d_top;                       // explain: the slices of both forms; pw, pg, term
    DevBuf<uint32_t> d_topu;                                    // ... code, count
    DevBuf<int32_t> d_npres;
    HIPC(c, d_ranges.reserve(2 * N, 2 * N));
    HIPC(c, d_short.reserve(size_t(std::max<int64_t>(n_short, 1)), size_t(std::max<int64_t>(n_short, 1))));
    HIPC(c, d_long.reserve(size_t(std::max<int64_t>(long_cap, 1)), size_t(std::max<int64_t>(long_cap, 1))));
    HIPC(c, d_nn.reserve(N, N));
    HIPC(c, d_cnt.reserve(4, 4));
    HIPC(c, d_status.reserve(np * N, np * N));
    HIPC(c, d_val.reserve(N * (np + size_t(ncol)), N * (np + size_t(ncol))));
    HIPC(c, hipMemcpyAsync(d_ranges.p, ranges.data(), 2 * N * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (n_short) HIPC(c, hipMemcpyAsync(d_short.p, short_rows.data(), size_t(n_short) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (n_long) HIPC(c, hipMemcpyAsync(d_long.p, long_rows.data(), size_t(n_long) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemsetAsync(d_cnt.p, 0, 4 * sizeof(unsigned int), c->stream));

    RangeParams P = RangeParams();
    P.codes = B.d_codes.p; P.inv = B.d_inv.p; P.low = B.d_low.p; P.ig = c->d_ig.p; P.ranges = d_ranges.p;
    P.kmin = c->kmin; P.kmax = c->kmax; P.rip = rip ? 1u : 0u;
    P.status = d_status.p; P.nn = d_nn.p; P.kld = d_val.p; P.gc = d_val.p + np * N;
    if (rip) { P.pi = P.gc + N; P.si = P.gc + 2 * N; P.cri = P.gc + 3 * N; }
    PanelParams Q = PanelParams();
    if (panel) {
        for (int t = 0; t * FRISK_PANEL_TILE < c->panel_n; ++t) Q.tile[t] = c->panel_tile[t].p;
        Q.n_prof = c->panel_n;
        Q.plane = n;
        P.ig = nullptr;
    }

    ExplainParams E = ExplainParams();
    const size_t NS = ex ? N * size_t(ex->top_n) : 0;
    if (ex) {
        HIPC(c, d_top.reserve(3 * NS, 3 * NS));
        HIPC(c, d_topu.reserve(2 * NS, 2 * NS));
        HIPC(c, d_npres.reserve(N, N));
        E.top_n = ex->top_n; E.n_present = d_npres.p;
        E.code = d_topu.p; E.count = d_topu.p + NS;
        E.pw = d_top.p; E.pg = d_top.p + NS; E.term = d_top.p + 2 * NS;
    }

    // the long form's scratch: one slice of 32-bit tables per workgroup (350 KB at 1..8, 89 MB at K = 12), as many workgroups as
    // the device can spare scratch for.  The short rows of kmax = 8 may all be handed over, but hardly any is: they add a few
    // workgroups to the grid, not one each (the grid-stride loop takes whatever the list holds in the end).
    const int64_t stride = (c->nprof + 3) / 4 * 4;
    int64_t want = std::min<int64_t>(n_long + std::min<int64_t>(long_cap - n_long, FRISK_RANGE_HANDOVER_WGS), c->num_cu);
    const size_t slice_long = ex ? size_t(cap_long) * 12 : 0;   // explain: bytes of a long-form workgroup's slice
    if (long_cap) {
        if (size_t(want) * size_t(stride) > c->d_big.cap || slice_long) {
            size_t free_b = 0, total_b = 0;
            HIPC(c, hipMemGetInfo(&free_b, &total_b));
            const int64_t fit = int64_t((free_b / 2 + c->d_big.cap * 4) / (size_t(stride) * 4 + slice_long));
            want = std::max<int64_t>(1, std::min(want, fit));
        }
        HIPC(c, c->d_big.reserve(size_t(want) * size_t(stride)));
        HIPC(c, hipMemsetAsync(c->d_big.p, 0, size_t(want) * size_t(stride) * 4, c->stream));
    }

    const RangeLds L = range_lds(c->kmin, c->kmax);
    // kmax = 8: the order-8 table leaves room for one workgroup per CU; below, three (43.7 KB at 1..7).  The panel kernel holds
    // a tile's 24 ExactSums in registers (196 VGPRs: two waves per SIMD, i.e. one workgroup per CU at any kmax)
    const int per_cu = (k8 || panel) ? 1 : 3;
    const int grid = int(std::min<int64_t>(n_short, int64_t(c->num_cu) * per_cu));
    if (ex) {           // the short form's slices, then the long form's
        const size_t words_short = n_short ? size_t(grid) * size_t(cap_short) * 3 / 2 : 0;
        const size_t words_long = long_cap ? size_t(want) * size_t(cap_long) * 3 / 2 : 0;
        HIPC(c, d_stage.reserve(words_short + words_long + 1, words_short + words_long + 1));
        E.stage = d_stage.p;
    }

    HIPC(c, hipEventRecord(c->ev0, c->stream));
    if (ex) {
        explain_fill_kernel<<<grid_for(int64_t(NS), 256, 4096), 256, 0, c->stream>>>(E, n);
        HIPC(c, hipGetLastError());
    }
    if (n_short) {
        RangeParams S = P;
        S.list = d_short.p; S.n_list = n_short; S.more = nullptr;
        S.out_list = d_long.p + n_long; S.out_count = d_cnt.p;
        if (ex) {
            E.R = S; E.cap = cap_short;
            HIPC(c, k8 ? launch_explain_short<true>(E, grid, L.total, c->stream) : launch_explain_short<false>(E, grid, L.total, c->stream));
        } else if (panel) {
            Q.R = S;
            const size_t lds = panel_lds_total(c->kmin, c->kmax);
            HIPC(c, k8 ? launch_panel_short<true>(Q, grid, lds, c->stream) : launch_panel_short<false>(Q, grid, lds, c->stream));
        } else {
            HIPC(c, k8 ? launch_short<true>(S, grid, L.total, c->stream) : launch_short<false>(S, grid, L.total, c->stream));
        }
    }
    if (long_cap) {     // (kmax = 8 without a long row: a few workgroups that find the hand-over list empty nearly always)
        RangeParams G = P;
        G.list = d_long.p; G.n_list = n_long; G.more = (k8 && n_short) ? d_cnt.p : nullptr;
        if (ex) {
            E.R = G; E.cap = cap_long;
            E.stage = d_stage.p + (n_short ? size_t(grid) * size_t(cap_short) * 3 / 2 : 0);
            explain_long_kernel<<<int(want), FRISK_RANGE_BIG_NT, 0, c->stream>>>(E, c->d_big.p, stride);
        } else if (panel) {
            Q.R = G;
            panel_long_kernel<<<int(want), FRISK_RANGE_BIG_NT, 0, c->stream>>>(Q, c->d_big.p, stride);
        } else {
            range_long_kernel<<<int(want), FRISK_RANGE_BIG_NT, 0, c->stream>>>(G, c->d_big.p, stride);
        }
        HIPC(c, hipGetLastError());
    }
    HIPC(c, hipEventRecord(c->ev1, c->stream));
    HIPC(c, hipMemcpyAsync(status, d_status.p, np * N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(nn, d_nn.p, N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(kld, P.kld, np * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(gc, P.gc, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (rip) {
        HIPC(c, hipMemcpyAsync(pi, P.pi, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(si, P.si, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(cri, P.cri, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    if (ex) {
        HIPC(c, hipMemcpyAsync(ex->n_present, d_npres.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(ex->code, E.code, NS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(ex->count, E.count, NS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(ex->pw, E.pw, NS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(ex->pg, E.pg, NS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(ex->term, E.term, NS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPC(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->ms[ex ? 7 : panel ? 5 : 4] = ms;
    return FRISK_OK;
}

}  // namespace

extern "C" int frisk_score_ranges(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                  uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si, double* cri,
                                  int64_t* nn) {
    return score_ranges(c, false, nullptr, seq_index, start, stop, n, flags, status, kld, gc, pi, si, cri, nn);
}

extern "C" int frisk_explain_ranges(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                    uint32_t flags, int32_t top_n, uint32_t* status, double* kld, double* gc, double* pi, double* si,
                                    double* cri, int64_t* nn, int32_t* n_present, uint32_t* code, uint32_t* count, double* pw,
                                    double* pg, double* term) {
    const ExplainOut ex = {top_n, n_present, code, count, pw, pg, term};
    return score_ranges(c, false, &ex, seq_index, start, stop, n, flags, status, kld, gc, pi, si, cri, nn);
}

extern "C" int frisk_score_ranges_panel(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                        uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si,
                                        double* cri, int64_t* nn) {
    return score_ranges(c, true, nullptr, seq_index, start, stop, n, flags, status, kld, gc, pi, si, cri, nn);
}

extern "C" int32_t frisk_panel_size(const frisk_ctx* c) { return c ? c->panel_n : 0; }

extern "C" int frisk_panel_reset(frisk_ctx* c) {
    if (!c) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));       // nothing queued reads a tile when it goes
    for (DevBuf<double>& t : c->panel_tile) t.release();
    c->panel_n = 0;
    return FRISK_OK;
}

extern "C" int frisk_panel_push(frisk_ctx* c, int32_t* slot) {
    if (!c) return FRISK_E_ARG;
    if (!c->profile_final) return fail(c, FRISK_E_STATE, "frisk_panel_push: no finalised profile");
    if (c->panel_n >= FRISK_PANEL_MAX) return fail(c, FRISK_E_ARG, "frisk_panel_push: the panel is full (FRISK_PANEL_MAX profiles)");
    HIPC(c, hipSetDevice(c->device));
    const int64_t nk = int64_t(1) << (2 * c->kmax);
    DevBuf<double>& tile = c->panel_tile[c->panel_n / FRISK_PANEL_TILE];
    const int at = c->panel_n % FRISK_PANEL_TILE;
    if (at == 0) HIPC(c, tile.reserve(size_t(nk) * FRISK_PANEL_TILE, size_t(nk) * FRISK_PANEL_TILE));
    // in stream order behind the kernel that finalised the table; a later profile call queues behind this copy
    panel_store_kernel<<<grid_for(nk, 256, 4096), 256, 0, c->stream>>>(c->d_ig.p, tile.p, nk, at, at == 0 ? 1 : 0);
    HIPC(c, hipGetLastError());
    if (slot) *slot = c->panel_n;
    ++c->panel_n;
    return FRISK_OK;
}
