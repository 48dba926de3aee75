// frisk_ranges.hip - the region scorer of the C ABI (include/frisk_hip.h): frisk_score_ranges, frisk_score_ranges_panel and
// frisk_explain_ranges - the scan loop's columns (KLD, GC, RIP indices) of arbitrary ranges of the resident batch against the
// context's finalised profile (range_kernels.h), against every profile of its panel in one pass (panel_kernels.h), and with the
// largest KLD terms of each range (explain_kernels.h) -, the panel's three calls, and frisk_refine_ranges, which moves a range's
// boundaries to the base (refine_kernels.h).  What the host decides is range_plan.h's: the
// row checks, the rows longest first (the workgroups of a launch take its list by grid stride) and their split between the two
// forms.  An entry point checks its call, plans it, and composes the steps below with its own kernels, buffers and timing slot:
// upload the plan, reserve the long form's scratch, queue both launches on the context's stream - a range the short form cannot
// hold reaches the long form through a device list, without a host round trip -, copy the columns back.  The context is
// frisk_ctx.h's; the scan's plan and row buffers are not touched.  gfx950 (MI355X) only.  Build: see __graft_entry__.build_hip().
#include <algorithm>

#include "frisk_ctx.h"
#include "range_plan.h"
#include "range_kernels.h"
#include "panel_kernels.h"
#include "explain_kernels.h"
#include "refine_kernels.h"

namespace {

// a short-form launch, the K = 8 instantiation or the other: the dynamic LDS is beyond the default limit
template <typename KERNEL, typename PARAMS>
hipError_t launch_with_lds(frisk_ctx* c, KERNEL kernel_k8, KERNEL kernel, const PARAMS& params, int grid, size_t lds) {
    if (c->kmax == 8) kernel = kernel_k8;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
    kernel<<<grid, FRISK_RANGE_NT, lds, c->stream>>>(params);
    return hipGetLastError();
}

// the arguments the three entry points share
struct RangeCall {
    const int32_t* seq_index;
    const int64_t *start, *stop;
    int64_t n;
    uint32_t flags;
    uint32_t* status;
    double *kld, *gc, *pi, *si, *cri;
    int64_t* nn;
    bool scored = true;         // the call returns kld and gc (frisk_refine_ranges does not)
    bool rip() const { return (flags & FRISK_SCAN_RIP) != 0; }
    bool arrays_given() const {
        return seq_index && start && stop && status && nn && (!scored || (kld && gc && (!rip() || (pi && si && cri))));
    }
};

// the device side of a call: the plan's arrays and the score columns (freed on every return)
struct RangeBufs {
    DevBuf<int64_t> ranges, short_rows, long_rows, nn;
    DevBuf<unsigned int> cnt;           // [0]: rows handed over to the long form
    DevBuf<uint32_t> status;            // `planes` planes
    DevBuf<double> val;                 // `planes` planes of kld, then gc [pi si cri]
};

// What every entry point checks before it plans: the call's own refusal (`early`, nullptr without), the resident batch, the
// flags, the state the entry point needs (`state_ok`, else FRISK_E_STATE with `state_msg`) and the arrays.  FRISK_OK: go on;
// RANGE_NOTHING_TO_DO: n = 0, the entry point returns FRISK_OK; else the refusal.
enum { RANGE_NOTHING_TO_DO = 1 };
int check_call(frisk_ctx* c, const std::string& who, const RangeCall& A, const char* early, bool state_ok, const char* state_msg,
               bool more_arrays_given) {
    if (A.n < 0) return fail(c, FRISK_E_ARG, who + ": n < 0");
    if (early) return fail(c, FRISK_E_ARG, who + early);
    const frisk_ctx::Batch& B = c->b();
    if (!B.have_seq) return fail(c, FRISK_E_ARG, who + ": no resident sequence batch");
    if (B.tiled) return fail(c, FRISK_E_ARG, who + ": the resident batch holds tiles, not whole scaffolds");
    if (A.rip() && !(c->kmin <= 2 && c->kmax >= 2)) return fail(c, FRISK_E_ARG, "FRISK_SCAN_RIP needs kmin <= 2 <= kmax");
    if (!state_ok) return fail(c, FRISK_E_STATE, who + state_msg);
    if (A.n == 0) return RANGE_NOTHING_TO_DO;
    if (!A.arrays_given() || !more_arrays_given) return fail(c, FRISK_E_ARG, who + ": null array");
    return FRISK_OK;
}

// Plan the call's rows (range_plan.h; a bad row is refused here), then take the device and wait for a streamed batch.
// per_cu_short: three workgroups of the short form per CU below kmax = 8 (43.7 KB of LDS at 1..7); one for a kernel that is held
// to one by its registers
int begin_call(frisk_ctx* c, const std::string& who, const RangeCall& A, int per_cu_short, int top_n, RangePlan& plan) {
    const frisk_ctx::Batch& B = c->b();
    const bool all_long = (A.flags & FRISK_RANGES_BIG) != 0 || c->kmax > 8;
    plan = plan_ranges(B.n_seq, B.seq_len.data(), B.seq_off.data(), A.seq_index, A.start, A.stop, A.n, c->kmax, all_long, c->num_cu,
                       per_cu_short, top_n);
    if (plan.error_code) return fail(c, plan.error_code, who + ": " + plan.error);
    HIPC(c, hipSetDevice(c->device));
    return settle_stream(c);
}

// Reserve the buffers, queue the copies of the plan's arrays and clear the hand-over counter; P: the kernels' common arguments,
// with `planes` planes of status and kld (the first at P.status / P.kld).
int upload_plan(frisk_ctx* c, const RangeCall& A, const RangePlan& plan, size_t planes, RangeBufs& D, RangeParams& P) {
    const frisk_ctx::Batch& B = c->b();
    const size_t N = size_t(A.n);
    const size_t ncol = A.rip() ? 4 : 1;
    const size_t n_short = size_t(plan.n_short()), n_long = size_t(plan.n_long()), long_cap = size_t(plan.long_cap);
    HIPC(c, D.ranges.reserve(2 * N, 2 * N));
    HIPC(c, D.short_rows.reserve(std::max<size_t>(n_short, 1), std::max<size_t>(n_short, 1)));
    HIPC(c, D.long_rows.reserve(std::max<size_t>(long_cap, 1), std::max<size_t>(long_cap, 1)));
    HIPC(c, D.nn.reserve(N, N));
    HIPC(c, D.cnt.reserve(4, 4));
    HIPC(c, D.status.reserve(planes * N, planes * N));
    HIPC(c, D.val.reserve(N * (planes + ncol), N * (planes + ncol)));
    HIPC(c, hipMemcpyAsync(D.ranges.p, plan.ranges.data(), 2 * N * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (n_short) HIPC(c, hipMemcpyAsync(D.short_rows.p, plan.short_rows.data(), n_short * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (n_long) HIPC(c, hipMemcpyAsync(D.long_rows.p, plan.long_rows.data(), n_long * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemsetAsync(D.cnt.p, 0, 4 * sizeof(unsigned int), c->stream));
    P = RangeParams();
    P.codes = B.d_codes.p; P.inv = B.d_inv.p; P.low = B.d_low.p; P.ig = c->d_ig.p; P.ranges = D.ranges.p;
    P.kmin = c->kmin; P.kmax = c->kmax; P.rip = A.rip() ? 1u : 0u;
    P.status = D.status.p; P.nn = D.nn.p; P.kld = D.val.p; P.gc = D.val.p + planes * N;
    if (A.rip()) { P.pi = P.gc + N; P.si = P.gc + 2 * N; P.cri = P.gc + 3 * N; }
    return FRISK_OK;
}

// the two launches' lists: the short form appends behind the long form's own rows
RangeParams short_list(RangeParams P, const RangePlan& plan, const RangeBufs& D) {
    P.list = D.short_rows.p; P.n_list = plan.n_short(); P.more = nullptr;
    P.out_list = D.long_rows.p + plan.n_long(); P.out_count = D.cnt.p;
    return P;
}
RangeParams long_list(RangeParams P, const RangePlan& plan, const RangeBufs& D) {
    P.list = D.long_rows.p; P.n_list = plan.n_long();
    P.more = plan.long_cap > plan.n_long() ? D.cnt.p : nullptr;     // (kmax = 8 with short rows)
    return P;
}

// The long form's scratch: one slice of `stride` 32-bit words per workgroup (350 KB at 1..8, 89 MB at K = 12) in the context's
// d_big, all-zero, for as many workgroups (`wgs`) as the device can spare scratch for; slice_bytes: what a workgroup needs beside
// it.  Nothing without a long-form launch.
int reserve_long_scratch(frisk_ctx* c, const RangePlan& plan, size_t slice_bytes, int64_t& wgs, int64_t& stride) {
    stride = (c->nprof + 3) / 4 * 4;
    wgs = plan.want_long;
    if (!plan.long_cap) return FRISK_OK;
    if (size_t(wgs) * size_t(stride) > c->d_big.cap || slice_bytes) {
        size_t free_b = 0, total_b = 0;
        HIPC(c, hipMemGetInfo(&free_b, &total_b));
        wgs = fit_long_workgroups(wgs, stride, slice_bytes, free_b, c->d_big.cap);
    }
    HIPC(c, c->d_big.reserve(size_t(wgs) * size_t(stride)));
    HIPC(c, hipMemsetAsync(c->d_big.p, 0, size_t(wgs) * size_t(stride) * 4, c->stream));
    return FRISK_OK;
}

// end of the timed interval; the score columns to the caller's arrays (queued)
int copy_back(frisk_ctx* c, const RangeCall& A, const RangeParams& P, size_t planes) {
    const size_t N = size_t(A.n);
    HIPC(c, hipEventRecord(c->ev1, c->stream));
    HIPC(c, hipMemcpyAsync(A.status, P.status, planes * N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(A.nn, P.nn, N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(A.kld, P.kld, planes * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(A.gc, P.gc, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (A.rip()) {
        HIPC(c, hipMemcpyAsync(A.pi, P.pi, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(A.si, P.si, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(A.cri, P.cri, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    return FRISK_OK;
}

// wait for the call; the kernels' time between the two events goes to frisk_last_kernel_ms(ctx, slot)
int finish_call(frisk_ctx* c, int slot) {
    HIPC(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPC(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->ms[slot] = ms;
    return FRISK_OK;
}

}  // namespace

extern "C" int frisk_score_ranges(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                  uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si, double* cri,
                                  int64_t* nn) {
    if (!c) return FRISK_E_ARG;
    const std::string who = "frisk_score_ranges";
    const RangeCall A = {seq_index, start, stop, n, flags, status, kld, gc, pi, si, cri, nn};
    if (int rc = check_call(c, who, A, nullptr, c->profile_final, ": no finalised profile", true)) return rc == RANGE_NOTHING_TO_DO ? FRISK_OK : rc;
    RangePlan plan;
    if (int rc = begin_call(c, who, A, 3, 0, plan)) return rc;
    RangeBufs D;
    RangeParams P;
    int64_t wgs = 0, stride = 0;
    if (int rc = upload_plan(c, A, plan, 1, D, P)) return rc;
    if (int rc = reserve_long_scratch(c, plan, 0, wgs, stride)) return rc;
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    if (plan.n_short()) {
        const size_t lds = range_lds(c->kmin, c->kmax).total;
        const RangeParams S = short_list(P, plan, D);
        HIPC(c, launch_with_lds(c, range_short_kernel<true>, range_short_kernel<false>, S, plan.grid_short, lds));
    }
    if (plan.long_cap) {        // (kmax = 8 without a long row: a few workgroups that find the hand-over list empty nearly always)
        range_long_kernel<<<int(wgs), FRISK_RANGE_BIG_NT, 0, c->stream>>>(long_list(P, plan, D), c->d_big.p, stride);
        HIPC(c, hipGetLastError());
    }
    if (int rc = copy_back(c, A, P, 1)) return rc;
    return finish_call(c, 4);
}

extern "C" int frisk_score_ranges_panel(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                        uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si,
                                        double* cri, int64_t* nn) {
    if (!c) return FRISK_E_ARG;
    const std::string who = "frisk_score_ranges_panel";
    const RangeCall A = {seq_index, start, stop, n, flags, status, kld, gc, pi, si, cri, nn};
    if (int rc = check_call(c, who, A, nullptr, c->panel_n != 0, ": the panel is empty", true)) return rc == RANGE_NOTHING_TO_DO ? FRISK_OK : rc;
    // the short kernel holds a tile's 24 ExactSums in registers (196 VGPRs: two waves per SIMD, i.e. one workgroup per CU at any kmax)
    RangePlan plan;
    if (int rc = begin_call(c, who, A, 1, 0, plan)) return rc;
    RangeBufs D;
    PanelParams Q = PanelParams();
    int64_t wgs = 0, stride = 0;
    if (int rc = upload_plan(c, A, plan, size_t(c->panel_n), D, Q.R)) return rc;
    Q.R.ig = nullptr;           // the tiles take its place
    for (int t = 0; t * FRISK_PANEL_TILE < c->panel_n; ++t) Q.tile[t] = c->panel_tile[t].p;
    Q.n_prof = c->panel_n;
    Q.plane = n;
    const RangeParams P = Q.R;
    if (int rc = reserve_long_scratch(c, plan, 0, wgs, stride)) return rc;
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    if (plan.n_short()) {
        const size_t lds = panel_lds_total(c->kmin, c->kmax);
        Q.R = short_list(P, plan, D);
        HIPC(c, launch_with_lds(c, panel_short_kernel<true>, panel_short_kernel<false>, Q, plan.grid_short, lds));
    }
    if (plan.long_cap) {
        Q.R = long_list(P, plan, D);
        panel_long_kernel<<<int(wgs), FRISK_RANGE_BIG_NT, 0, c->stream>>>(Q, c->d_big.p, stride);
        HIPC(c, hipGetLastError());
    }
    if (int rc = copy_back(c, A, P, size_t(c->panel_n))) return rc;
    return finish_call(c, 5);
}

extern "C" int frisk_explain_ranges(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                    uint32_t flags, int32_t top_n, uint32_t* status, double* kld, double* gc, double* pi, double* si,
                                    double* cri, int64_t* nn, int32_t* n_present, uint32_t* code, uint32_t* count, double* pw,
                                    double* pg, double* term) {
    if (!c) return FRISK_E_ARG;
    const std::string who = "frisk_explain_ranges";
    const RangeCall A = {seq_index, start, stop, n, flags, status, kld, gc, pi, si, cri, nn};
    const char* bad_top = top_n < 1 || top_n > FRISK_EXPLAIN_MAX ? ": top_n outside 1 .. FRISK_EXPLAIN_MAX" : nullptr;
    if (int rc = check_call(c, who, A, bad_top, c->profile_final, ": no finalised profile", n_present && code && count && pw && pg && term)) return rc == RANGE_NOTHING_TO_DO ? FRISK_OK : rc;
    RangePlan plan;
    if (int rc = begin_call(c, who, A, 3, top_n, plan)) return rc;
    RangeBufs D;
    DevBuf<double> d_stage, d_top;      // the slices of both forms; pw, pg, term
    DevBuf<uint32_t> d_topu;            // code, count
    DevBuf<int32_t> d_npres;
    ExplainParams E = ExplainParams();
    int64_t wgs = 0, stride = 0;
    if (int rc = upload_plan(c, A, plan, 1, D, E.R)) return rc;
    const RangeParams P = E.R;
    const size_t N = size_t(n), NS = N * size_t(top_n);
    HIPC(c, d_top.reserve(3 * NS, 3 * NS));
    HIPC(c, d_topu.reserve(2 * NS, 2 * NS));
    HIPC(c, d_npres.reserve(N, N));
    E.top_n = top_n; E.n_present = d_npres.p;
    E.code = d_topu.p; E.count = d_topu.p + NS;
    E.pw = d_top.p; E.pg = d_top.p + NS; E.term = d_top.p + 2 * NS;
    // a slice entry is 12 bytes: a term and a 32-bit code.  The short form's slices, then the long form's
    if (int rc = reserve_long_scratch(c, plan, size_t(plan.cap_long) * 12, wgs, stride)) return rc;
    const size_t words_short = plan.n_short() ? size_t(plan.grid_short) * size_t(plan.cap_short) * 3 / 2 : 0;
    const size_t words_long = plan.long_cap ? size_t(wgs) * size_t(plan.cap_long) * 3 / 2 : 0;
    HIPC(c, d_stage.reserve(words_short + words_long + 1, words_short + words_long + 1));
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    explain_fill_kernel<<<grid_for(int64_t(NS), 256, 4096), 256, 0, c->stream>>>(E, n);
    HIPC(c, hipGetLastError());
    if (plan.n_short()) {
        const size_t lds = range_lds(c->kmin, c->kmax).total;
        E.R = short_list(P, plan, D); E.cap = plan.cap_short; E.stage = d_stage.p;
        HIPC(c, launch_with_lds(c, explain_short_kernel<true>, explain_short_kernel<false>, E, plan.grid_short, lds));
    }
    if (plan.long_cap) {
        E.R = long_list(P, plan, D); E.cap = plan.cap_long; E.stage = d_stage.p + words_short;
        explain_long_kernel<<<int(wgs), FRISK_RANGE_BIG_NT, 0, c->stream>>>(E, c->d_big.p, stride);
        HIPC(c, hipGetLastError());
    }
    if (int rc = copy_back(c, A, P, 1)) return rc;
    HIPC(c, hipMemcpyAsync(n_present, d_npres.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(code, E.code, NS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(count, E.count, NS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(pw, E.pw, NS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(pg, E.pg, NS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(term, E.term, NS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return finish_call(c, 7);
}

extern "C" int frisk_refine_ranges(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n,
                                   uint32_t flags, int32_t flank, int32_t order, uint32_t* status, int64_t* nn, int64_t* new_start,
                                   int64_t* new_stop, int64_t* gain_start, int64_t* gain_stop, int64_t* flank_used) {
    if (!c) return FRISK_E_ARG;
    const std::string who = "frisk_refine_ranges";
    const RangeCall A = {seq_index, start, stop, n, flags & FRISK_RANGES_BIG, status, nullptr, nullptr, nullptr, nullptr, nullptr, nn, false};
    const char* bad = refine_args_problem(flank, order, c->kmin, c->kmax);
    const std::string early = bad ? std::string(": ") + bad : std::string();
    if (int rc = check_call(c, who, A, bad ? early.c_str() : nullptr, c->profile_final, ": no finalised profile",
                            new_start && new_stop && gain_start && gain_stop && flank_used)) return rc == RANGE_NOTHING_TO_DO ? FRISK_OK : rc;
    // the rows of the range kernels are the cores (range_plan.h: plan_refine).  Two workgroups of the short form per CU below
    // kmax = 8: the mode's table takes 8 KB of LDS beside the form's
    const frisk_ctx::Batch& B = c->b();
    const bool all_long = (A.flags & FRISK_RANGES_BIG) != 0 || c->kmax > 8;
    const RefinePlan R = plan_refine(B.n_seq, B.seq_len.data(), B.seq_off.data(), seq_index, start, stop, n, flank, order, c->kmin, c->kmax,
                                     all_long, c->num_cu, 2);
    const RangePlan& plan = R.plan;
    if (plan.error_code) return fail(c, plan.error_code, who + ": " + plan.error);
    HIPC(c, hipSetDevice(c->device));
    if (int rc = settle_stream(c)) return rc;
    RangeBufs D;
    DevBuf<int64_t> d_geom, d_host, d_out;
    RefineParams E = RefineParams();
    int64_t wgs = 0, stride = 0;
    if (int rc = upload_plan(c, A, plan, 1, D, E.R)) return rc;         // (kld and gc of the cores: written, not returned)
    const RangeParams P = E.R;
    const size_t N = size_t(n), n_words = size_t(1) << (2 * (order + 1));
    HIPC(c, d_geom.reserve(R.geom.size(), R.geom.size()));
    HIPC(c, d_host.reserve(n_words, n_words));
    HIPC(c, d_out.reserve(5 * N, 5 * N));
    HIPC(c, hipMemcpyAsync(d_geom.p, R.geom.data(), R.geom.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    E.geom = d_geom.p; E.host_lp = d_host.p; E.order = order;
    E.new_start = d_out.p; E.new_stop = d_out.p + N; E.gain_start = d_out.p + 2 * N; E.gain_stop = d_out.p + 3 * N;
    E.flank_used = d_out.p + 4 * N;
    if (int rc = reserve_long_scratch(c, plan, 0, wgs, stride)) return rc;
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    refine_host_kernel<<<grid_for(int64_t(n_words), 256, c->num_cu * 8), 256, 0, c->stream>>>(c->d_sym.p + table_offset(c->kmin, order + 1),
                                                                                           int64_t(n_words), d_host.p);
    HIPC(c, hipGetLastError());
    if (plan.n_short()) {
        const size_t lds = range_lds(c->kmin, c->kmax).total;
        E.R = short_list(P, plan, D);
        HIPC(c, launch_with_lds(c, refine_short_kernel<true>, refine_short_kernel<false>, E, plan.grid_short, lds));
    }
    if (plan.long_cap) {
        E.R = long_list(P, plan, D);
        refine_long_kernel<<<int(wgs), FRISK_RANGE_BIG_NT, 0, c->stream>>>(E, c->d_big.p, stride);
        HIPC(c, hipGetLastError());
    }
    HIPC(c, hipEventRecord(c->ev1, c->stream));
    HIPC(c, hipMemcpyAsync(status, P.status, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(nn, P.nn, N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    int64_t* const out[5] = {new_start, new_stop, gain_start, gain_stop, flank_used};
    for (size_t k = 0; k < 5; ++k) HIPC(c, hipMemcpyAsync(out[k], d_out.p + k * N, N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    return finish_call(c, 8);
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
