// frisk_abi.hip - host side of libfrisk_hip.so: the context's creation and destruction, its small getters, the profile (phase A: its
// launches are planned in profile_plan.h) and the scan of the C ABI declared in include/frisk_hip.h.  The context itself is
// frisk_ctx.h's; the sequence and FASTA entry points are in frisk_seq.hip.  The scan kernels are launched through scan_launch.h (scan_launch.hip, scan8_launch*.hip), each by the form that the schedule names; the
// entry points that take no context (HMM, projection, clustering) are in frisk_analysis.hip.  gfx950 (MI355X) only.  Build: see
// __graft_entry__.build_hip().
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "frisk_ctx.h"
#include "profile_kernels.h"
#include "profile_plan.h"
#include "scan_launch.h"
#include "scan_schedule.h"
#include "scan_tiles.h"             // plan_scaffold
#include "ring_rows.h"              // FRISK8_RING_COLS
#include "table_text.h"

namespace {

int64_t profile_len(int kmin, int kmax) { return table_offset(kmin, kmax + 1); }

// Tuning knobs are read from the environment only in experiment builds (-DFRISK_TUNE); the product library has none.
inline const char* tune_env(const char* name) {
#ifdef FRISK_TUNE
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

int build_genome_table(frisk_ctx* c) {
    const int64_t n = int64_t(1) << (2 * c->kmax);
    genome_ivom_kernel<<<grid_for(n, 256, 1 << 20), 256, 0, c->stream>>>(c->d_sym.p, c->kmin, c->kmax, c->d_meta.p, c->d_ig.p);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(c->h_meta.p, c->d_meta.p, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    ++c->ig_gen;                    // (the copy of the table that heads the scan's ring buffer is stale)
    c->profile_final = true;        // in stream order: everything that follows on the context's stream sees the table
    return FRISK_OK;
}

}  // namespace

extern "C" {

const char* frisk_version(void) { return "frisk_hip 0.1 (gfx950)"; }

int frisk_supported(int kmin, int kmax, int64_t max_window) {
    return (kmin >= 1 && kmin <= kmax && kmax <= FRISK_MAX_K && max_window >= 1 && max_window <= 0x7FFFFFFF) ? 1 : 0;
}

int frisk_create(int device, int kmin, int kmax, frisk_ctx** out) {
    if (!out) return FRISK_E_ARG;
    *out = nullptr;
    frisk_ctx* c = new (std::nothrow) frisk_ctx();
    if (!c) return FRISK_E_HIP;
    *out = c;       // returned even on failure so that frisk_last_error() can be read; caller destroys it
    if (kmin < 1 || kmin > kmax || kmax > FRISK_MAX_K)
        return fail(c, FRISK_E_ARG, "word sizes must satisfy 1 <= kmin <= kmax <= 12");
    c->device = device;
    c->kmin = kmin;
    c->kmax = kmax;
    c->nprof = profile_len(kmin, kmax);
    int ndev = 0;
    HIPC(c, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(c, FRISK_E_HIP, "no such HIP device");
    HIPC(c, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPC(c, hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(c, FRISK_E_HIP, std::string("libfrisk_hip is built for gfx950 only; device is ") + prop.gcnArchName);
    c->num_cu = prop.multiProcessorCount;
    HIPC(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPC(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIPC(c, hipEventCreateWithFlags(&c->staged_ev, hipEventDisableTiming));
    HIPC(c, hipEventCreateWithFlags(&c->slot_free_ev, hipEventDisableTiming));
    HIPC(c, hipStreamCreateWithFlags(&c->tail_stream, hipStreamNonBlocking));
    HIPC(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPC(c, hipEventCreateWithFlags(&c->ev_tail_kernels, hipEventDisableTiming));
    HIPC(c, hipEventCreateWithFlags(&c->ev_tail_done, hipEventDisableTiming));
    HIPC(c, hipEventCreate(&c->ev0));
    HIPC(c, hipEventCreate(&c->ev1));
    HIPC(c, c->d_raw.reserve(size_t(c->nprof) + 4));
    HIPC(c, c->d_cnt.reserve(size_t(c->nprof) + 4));
    HIPC(c, c->d_sym.reserve(size_t(c->nprof)));
    HIPC(c, c->d_ig.reserve(size_t(1) << (2 * kmax)));
    HIPC(c, c->d_meta.reserve(4));
    HIPC(c, c->h_meta.reserve(4, 4));
    HIPC(c, hipEventCreate(&c->evp0));
    HIPC(c, hipEventCreate(&c->evp1));
    HIPC(c, hipMemsetAsync(c->d_raw.p, 0, (size_t(c->nprof) + 4) * sizeof(int64_t), c->stream));
    {   // range-reduction table of the scan kernel's logarithm (scan_kernel.h: log_tab_pos)
        double tab[2 * FRISK_LOGTAB_N];
        for (int nbin : {FRISK_LOGTAB_N, 64, 32}) {
            for (int i = 0; i < nbin; ++i) {
                const double ci = 0.5 + (double(i) + 0.5) / (2.0 * nbin);
                const double u = 1.0 / ci;
                tab[2 * i] = u;
                tab[2 * i + 1] = double(-logl((long double)u));      // -ln of the ROUNDED reciprocal: the identity stays exact
            }
            DevBuf<double>& dst = nbin == 64 ? c->d_logtab64 : (nbin == 32 ? c->d_logtab32 : c->d_logtab);
            HIPC(c, dst.reserve(2 * size_t(nbin)));
            HIPC(c, hipMemcpyAsync(dst.p, tab, 2 * size_t(nbin) * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIPC(c, hipStreamSynchronize(c->stream));                // `tab` is reused
        }
        double rc[256];                                          // scan8_kernel.h: weight 1/c of a position whose max-mer occurs c times
        rc[0] = 0.0;
        for (int i = 1; i < 256; ++i) rc[i] = 1.0 / double(i);
        HIPC(c, c->d_rctab.reserve(256));
        HIPC(c, hipMemcpyAsync(c->d_rctab.p, rc, sizeof(rc), hipMemcpyHostToDevice, c->stream));
        HIPC(c, c->d_ovf_count.reserve(SCAN_CNT_TOTAL));
        HIPC(c, c->d_verdict.reserve(8));
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    return FRISK_OK;
}

void frisk_destroy(frisk_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // nothing of the context's is in flight when its memory goes: all three streams, and the DMAs out of the staging pieces
    const hipStream_t streams[] = {c->stream, c->copy_stream, c->tail_stream};
    for (hipStream_t s : streams) if (s) (void)hipStreamSynchronize(s);
    for (hipEvent_t e : c->pin_ev) if (e) (void)hipEventSynchronize(e);
    for (hipStream_t s : streams) if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : {c->ev0, c->ev1, c->evp0, c->evp1, c->evn0, c->evn1, c->staged_ev, c->slot_free_ev, c->ev_fork, c->ev_tail_kernels, c->ev_tail_done})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->pin_ev) if (e) (void)hipEventDestroy(e);
    delete c;       // device and page-locked memory and the batches' piece events go with their owners (frisk_ctx.h)
}

const char* frisk_last_error(const frisk_ctx* c) { return c ? c->err.c_str() : "null context"; }
int64_t frisk_profile_len(const frisk_ctx* c) { return c ? c->nprof : 0; }
int64_t frisk_profile_raw_len(const frisk_ctx* c) { return c ? c->nprof + 4 : 0; }
int64_t frisk_seq_padded_len(const frisk_ctx* c) { return (c && c->b().have_seq) ? c->b().padded_len : 0; }
void* frisk_host_alloc(frisk_ctx* c, int64_t bytes) {
    if (!c || bytes <= 0) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    if (hipHostMalloc(&p, size_t(bytes), hipHostMallocDefault) != hipSuccess) { c->err = "hipHostMalloc failed"; return nullptr; }
    return p;
}
void frisk_host_free(frisk_ctx* c, void* ptr) {
    if (c && ptr) { (void)hipSetDevice(c->device); (void)hipHostFree(ptr); }
}
double frisk_last_kernel_ms(const frisk_ctx* cc, int which) {
    frisk_ctx* c = const_cast<frisk_ctx*>(cc);
    if (!c || which < 0 || which >= 9) return -1.0;
    if (which == 1 && c->ms_pending[1]) {           // the profile kernel's events are read on demand: no sync in profile_add
        float ms = 0;
        if (hipEventSynchronize(c->evp1) == hipSuccess && hipEventElapsedTime(&ms, c->evp0, c->evp1) == hipSuccess) c->ms[1] = ms;
        c->ms_pending[1] = false;
    }
    return c->ms[which];
}

// --------------------------------------------------------------------------------------- phase A
int frisk_profile_reset(frisk_ctx* c) {
    if (!c) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemsetAsync(c->d_raw.p, 0, (size_t(c->nprof) + 4) * sizeof(int64_t), c->stream));
    c->profile_final = false;
    return FRISK_OK;
}

static int profile_add_range(frisk_ctx* c, int mask_host, bool one_pass, int64_t p0, int64_t p1, bool first = true, bool last = true);
static int launch_profile(frisk_ctx* c, const ProfileLaunch& L, int mask_host, int64_t p0, int64_t p1, bool first, bool last);

int frisk_profile_add(frisk_ctx* c, int mask_host, int64_t p0, int64_t p1) {
    if (!c) return FRISK_E_ARG;
    // the flags split before any branch: every form below is handed --maskHost (bit 0) alone, the one-pass hook on its own
    const bool one_pass = (mask_host & FRISK_PROFILE_ONE_PASS) != 0;
    mask_host &= 1;
    if (!c->b().have_seq) return fail(c, FRISK_E_STATE, "frisk_profile_add: no resident sequence batch");
    if (c->b().tiled) {
        // a tiled batch: "the whole batch" means the positions this rank OWNS (every base of the genome is owned by exactly
        // one rank; the K-1 bases kept behind an owned range belong to the words that start inside it)
        if (!(p0 < 0 && p1 < 0)) return fail(c, FRISK_E_ARG, "frisk_profile_add: a tiled batch is profiled as a whole (-1, -1)");
        c->profile_final = false;           // (as every add: also when this rank owns no position)
        const frisk_ctx::Batch& B = c->b();
        for (size_t t = 0; t < B.tiles.size(); ++t) {
            const frisk_ctx::Batch::Tile& T = B.tiles[t];
            if (T.own1 <= T.own0) continue;
            int rc = profile_add_range(c, mask_host, one_pass, B.seq_off[t] + (T.own0 - T.base0), B.seq_off[t] + (T.own1 - T.base0));
            if (rc) return rc;
        }
        return FRISK_OK;
    }
    frisk_ctx::Batch& SB = c->b();
    if (SB.streaming && p0 < 0 && p1 < 0 && !SB.piece_end.empty()) {
        // a streamed batch counted as a whole: phase A follows the copies piece by piece (plan_profile_pieces), each launch behind
        // the events of the pieces it reads
        HIPC(c, hipSetDevice(c->device));
        size_t waited = 0;
        for (const ProfilePiece& L : plan_profile_pieces(SB.piece_end, SB.padded_len)) {
            for (; waited <= L.piece; ++waited) HIPC(c, hipStreamWaitEvent(c->stream, SB.piece_ev[waited], 0));
            int rc = profile_add_range(c, mask_host, one_pass, L.p0, L.p1, L.first, L.last);
            if (rc) return rc;
        }
        SB.streaming = false;
        return FRISK_OK;
    }
    if (int rs = settle_stream(c)) return rs;
    return profile_add_range(c, mask_host, one_pass, p0, p1);
}

static int profile_add_range(frisk_ctx* c, int mask_host, bool one_pass, int64_t p0, int64_t p1, bool first, bool last) {
    if (p0 < 0 && p1 < 0) { p0 = 0; p1 = c->b().padded_len; }
    if (p0 < 0 || p1 > c->b().padded_len || p0 > p1) return fail(c, FRISK_E_ARG, "position range outside the batch");
    HIPC(c, hipSetDevice(c->device));
    c->profile_final = false;
    return launch_profile(c, plan_profile_launch(c->kmax, c->num_cu, p0, p1, one_pass), mask_host ? 1 : 0, p0, p1, first, last);
}

// One planned launch (profile_plan.h) on the context's stream, between the events of frisk_last_kernel_ms(1): the start event with
// the first launch of a call, the end event with its last.  An empty range launches nothing; its events are recorded all the same.
static int launch_profile(frisk_ctx* c, const ProfileLaunch& L, int mask_host, int64_t p0, int64_t p1, bool first, bool last) {
    static_assert(PROFILE_LDS_THREADS == FRISK_PROF_NT, "the plan's workgroup is the kernels'");
    const frisk_ctx::Batch& B = c->b();
    const uint32_t *codes = B.d_codes.p, *inv = B.d_inv.p, *low = B.d_low.p;
    auto raw = reinterpret_cast<unsigned long long*>(c->d_raw.p);
    const int kmin = c->kmin, kmax = c->kmax, nprof = int(c->nprof);
    if (first) HIPC(c, hipEventRecord(c->evp0, c->stream));
    if (L.grid > 0) {
        const void* kernel = L.form == PROFILE_FORM_BIG ? reinterpret_cast<const void*>(profile_add_big_kernel)
                           : L.form == PROFILE_FORM_ONE_PASS ? reinterpret_cast<const void*>(profile_add16_kernel)
                                                             : reinterpret_cast<const void*>(profile_add_kernel);
        if (L.lds_bytes) HIPC(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(L.lds_bytes)));
        switch (L.form) {
            case PROFILE_FORM_BIG:
                profile_add_big_kernel<<<L.grid, L.threads, L.lds_bytes, c->stream>>>(codes, inv, low, p0, p1, kmin, kmax, mask_host, nprof, raw);
                break;
            case PROFILE_FORM_ONE_PASS:
                profile_add16_kernel<<<L.grid, L.threads, L.lds_bytes, c->stream>>>(codes, inv, low, p0, p1, kmin, mask_host, nprof, L.chunk_words, raw);
                break;
            case PROFILE_FORM_LDS:
                profile_add_kernel<<<L.grid, L.threads, L.lds_bytes, c->stream>>>(codes, inv, low, p0, p1, kmin, kmax, mask_host, nprof, L.halves,
                                                                                 L.chunk_words, raw);
                break;
        }
    }
    HIPC(c, hipGetLastError());
    if (last) {
        HIPC(c, hipEventRecord(c->evp1, c->stream));
        c->ms_pending[1] = true;    // asynchronous: the elapsed time is read when frisk_last_kernel_ms(1) asks for it
    }
    return FRISK_OK;
}

int frisk_profile_export_device(frisk_ctx* c, void* dst) {
    if (!c || !dst) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(dst, c->d_raw.p, (size_t(c->nprof) + 4) * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return FRISK_OK;
}
int frisk_profile_import_device(frisk_ctx* c, const void* src) {
    if (!c || !src) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(c->d_raw.p, src, (size_t(c->nprof) + 4) * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->profile_final = false;
    return FRISK_OK;
}
int frisk_profile_device_view(frisk_ctx* c, void** raw, void** stream) {
    if (!c || !raw || !stream) return FRISK_E_ARG;
    *raw = c->d_raw.p;
    *stream = reinterpret_cast<void*>(c->stream);
    c->profile_final = false;
    return FRISK_OK;
}
// The one collective of a multi-GPU job, without torch: RCCL's all-reduce(sum, int64) IN PLACE on the raw profile, on the context's
// stream.  librccl is not linked: the copy already in the process (PyTorch-ROCm brings its own under the same SONAME) or the
// system one is resolved on first use, so that a one-GPU process never loads it.
int frisk_profile_allreduce(frisk_ctx* c, void* rccl_comm) {
    if (!c) return FRISK_E_ARG;
    if (!rccl_comm) return FRISK_OK;                    // one GPU: nothing to sum
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    typedef const char* (*errstr_fn)(int);
    static allreduce_fn all_reduce = nullptr;
    static errstr_fn err_string = nullptr;
    if (!all_reduce) {
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);           // the instance the caller's communicator came from
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return fail(c, FRISK_E_HIP, std::string("frisk_profile_allreduce: librccl not found: ") + dlerror());
        all_reduce = reinterpret_cast<allreduce_fn>(dlsym(h, "ncclAllReduce"));
        err_string = reinterpret_cast<errstr_fn>(dlsym(h, "ncclGetErrorString"));
        if (!all_reduce) return fail(c, FRISK_E_HIP, "frisk_profile_allreduce: ncclAllReduce not found in librccl");
    }
    HIPC(c, hipSetDevice(c->device));
    const int rc = all_reduce(c->d_raw.p, c->d_raw.p, size_t(c->nprof) + 4, /* ncclInt64 */ 4, /* ncclSum */ 0, rccl_comm, c->stream);
    if (rc != 0) return fail(c, FRISK_E_HIP, std::string("ncclAllReduce: ") + (err_string ? err_string(rc) : "error"));
    c->profile_final = false;
    return FRISK_OK;
}

int frisk_profile_export_host(frisk_ctx* c, int64_t* dst) {
    if (!c || !dst) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(dst, c->d_raw.p, (size_t(c->nprof) + 4) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return FRISK_OK;
}
int frisk_profile_import_host(frisk_ctx* c, const int64_t* src) {
    if (!c || !src) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(c->d_raw.p, src, (size_t(c->nprof) + 4) * 8, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->profile_final = false;
    return FRISK_OK;
}

int frisk_profile_finalize(frisk_ctx* c) {
    if (!c) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    const size_t nraw = size_t(c->nprof) + 4;
    HIPC(c, hipMemcpyAsync(c->d_cnt.p, c->d_raw.p, nraw * 8, hipMemcpyDeviceToDevice, c->stream));
    int x = c->kmax - 1;
    for (; x >= c->kmin && x > 7; --x) {                // the wide levels (K > 8): one launch per order
        const int64_t n = int64_t(1) << (2 * x);
        marginalize_kernel<<<grid_for(n, 256, 1 << 20), 256, 0, c->stream>>>(c->d_cnt.p, c->kmin, x);
    }
    if (x >= c->kmin) marginalize_low_kernel<<<1, 1024, 0, c->stream>>>(c->d_cnt.p, c->kmin, x);       // orders <= 7: one launch
    symmetrize_kernel<<<grid_for(c->nprof, 256, 1 << 20), 256, 0, c->stream>>>(c->d_cnt.p, c->d_sym.p, c->kmin, c->kmax);
    HIPC(c, hipGetLastError());
    // metadata of L356-359 (totalLen, exMax, nnTotal): computed on the device, mirrored to the host asynchronously
    profile_meta_kernel<<<1, 1024, 0, c->stream>>>(c->d_cnt.p, c->d_raw.p + c->nprof, c->kmin, c->kmax, c->d_meta.p);
    HIPC(c, hipGetLastError());
    return build_genome_table(c);
}

int frisk_profile_get(frisk_ctx* c, int64_t* sym, int64_t* total_len, int64_t* ex_max, int64_t* nn_total) {
    if (!c) return FRISK_E_ARG;
    if (!c->profile_final) return fail(c, FRISK_E_STATE, "profile not finalised");
    HIPC(c, hipSetDevice(c->device));
    if (sym) HIPC(c, hipMemcpyAsync(sym, c->d_sym.p, size_t(c->nprof) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (total_len) *total_len = c->h_meta.p[0];
    if (ex_max) *ex_max = c->h_meta.p[1];
    if (nn_total) *nn_total = c->h_meta.p[2];
    return FRISK_OK;
}

int frisk_profile_set(frisk_ctx* c, const int64_t* sym, int64_t total_len, int64_t ex_max, int64_t nn_total) {
    if (!c || !sym) return FRISK_E_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));                   // h_meta may still be the target of an earlier mirror copy
    HIPC(c, hipMemcpyAsync(c->d_sym.p, sym, size_t(c->nprof) * 8, hipMemcpyHostToDevice, c->stream));
    c->h_meta.p[0] = total_len; c->h_meta.p[1] = ex_max; c->h_meta.p[2] = nn_total;
    HIPC(c, hipMemcpyAsync(c->d_meta.p, c->h_meta.p, 3 * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));                   // `sym` is the caller's: the copy must have left it
    return build_genome_table(c);
}

// --------------------------------------------------------------------------------------- phase B
int frisk_scan_plan(frisk_ctx* c, int32_t w, int32_t inc, uint32_t flags, int64_t* n_candidates) {
    if (!c) return FRISK_E_ARG;
    if (!c->b().have_seq) return fail(c, FRISK_E_STATE, "frisk_scan_plan: no resident sequence batch");
    if (w < 1 || inc < 1) return fail(c, FRISK_E_ARG, "window length and increment must be >= 1");
    const bool all = (flags & FRISK_SCAN_SCAFFOLDS_ALL) != 0;
    if (c->plan_w == w && c->plan_inc == inc && ((c->plan_flags ^ flags) & FRISK_SCAN_SCAFFOLDS_ALL) == 0) {
        if (n_candidates) *n_candidates = c->plan_ncand;
        return FRISK_OK;
    }
    HIPC(c, hipSetDevice(c->device));
    const frisk_ctx::Batch& B = c->b();
    if (B.tiled && (w != B.tile_w || inc != B.tile_inc || (flags & FRISK_SCAN_SCAFFOLDS_ALL) != B.tile_flags))
        return fail(c, FRISK_E_ARG, "the resident batch holds the tiles of another window geometry (frisk_fasta_load_shard)");
    c->h_desc.assign(size_t(B.n_seq) + 1, ScafDesc());
    int64_t cand = 0, maxwin = 0;
    for (int32_t s = 0; s < B.n_seq; ++s) {
        ScafDesc& d = c->h_desc[size_t(s)];
        d.off = B.seq_off[size_t(s)];
        d.cand0 = cand;
        d.pad_ = 0;
        if (B.tiled) {              // candidates are numbered from the rank's first one; the windows were chosen at load time
            const frisk_ctx::Batch::Tile& t = B.tiles[size_t(s)];
            d.size = t.size; d.base0 = t.base0; d.j0 = t.j0; d.ncand = t.ncand; d.kind = t.kind;
        } else {
            d.size = B.seq_len[size_t(s)];
            d.base0 = 0; d.j0 = 0;
            plan_scaffold(d.size, w, inc, all, d.ncand, d.kind);
        }
        if (d.ncand > 0) maxwin = std::max<int64_t>(maxwin, d.kind == 1 ? d.size : w);
        cand += d.ncand;
    }
    ScafDesc& sentinel = c->h_desc[size_t(B.n_seq)];       // keeps the binary search in range
    sentinel.off = B.padded_len; sentinel.size = 0; sentinel.cand0 = cand; sentinel.ncand = 0; sentinel.kind = 0;
    sentinel.base0 = 0; sentinel.j0 = 0; sentinel.pad_ = 0;
    if (maxwin > 0x7FFFFFFF) return fail(c, FRISK_E_ARG, "a window longer than 2^31-1 bases");
    HIPC(c, c->d_desc.reserve(c->h_desc.size()));
    HIPC(c, hipMemcpyAsync(c->d_desc.p, c->h_desc.data(), c->h_desc.size() * sizeof(ScafDesc), hipMemcpyHostToDevice,
                           c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->plan_w = w; c->plan_inc = inc; c->plan_flags = flags; c->plan_ncand = cand; c->plan_maxwin = maxwin;
    if (n_candidates) *n_candidates = cand;
    return FRISK_OK;
}

namespace {

// what the schedule's decisions read (scan_schedule.h), from the context and the call
ScanShape scan_shape_of(frisk_ctx* c, int64_t n, int32_t w, int32_t inc, uint32_t flags, bool debug) {
    ScanShape s = ScanShape();
    s.kmin = c->kmin; s.kmax = c->kmax; s.num_cu = c->num_cu; s.n = n; s.w = w; s.inc = inc; s.flags = flags;
    s.plan_maxwin = c->plan_maxwin;
    s.debug = debug; s.want_ivom = c->want_ivom != nullptr; s.rip = (flags & FRISK_SCAN_RIP) != 0;
    const frisk_ctx::Batch& B = c->b();
    s.width_hint = B.width_hint; s.hint_side = B.hint_side; s.hint_matches = B.hint_w == w && B.hint_inc == inc;
    s.lv_shared = shared_level(c->kmin, c->kmax);
    s.lds_shared = make_layout(c->kmin, c->kmax, scan_orphan_cap(c->plan_maxwin), s.lv_shared).total;
    s.lds_level0 = make_layout(c->kmin, c->kmax, scan_orphan_cap(c->plan_maxwin), 0).total;
    if (const char* ev = tune_env("FRISK_SCAN_CHUNK")) { s.has_scan_chunk = true; s.scan_chunk = std::atoll(ev); }
    if (const char* ev = tune_env("FRISK_K8_BITS")) { s.has_k8_bits = true; s.k8_bits = std::atoi(ev); }
    s.one_wg = tune_env("FRISK_ONE_WG") != nullptr;
    s.no_slide = tune_env("FRISK_NO_SLIDE") != nullptr; s.no_deal = tune_env("FRISK_NO_DEAL") != nullptr;
    s.one_segment = tune_env("FRISK_ONE_SEGMENT") != nullptr; s.tail_any = tune_env("FRISK_TAIL_ANY") != nullptr;
    return s;
}

// One frisk_scan between its schedule and its rows: the schedule (read, never decided, here), the kernel arguments of the whole
// range and the caller's buffers.  reserve(), enqueue() and collect() run once each, in this order.
struct ScanRun {
    frisk_ctx* c;
    const ScanShape& shape;
    const ScanSchedule& sched;
    int32_t* seq_index; int64_t* start; int64_t* stop; uint32_t* status; double* kld; double* gc; double* pi; double* si; double* cri;
    uint32_t* dbg_counts; int64_t* dbg_meta;
    ScanParams P;
    size_t nk;                              // 4^kmax
    unsigned int novf_sample[2];            // the sample's own hand-overs (its counters are cleared for the bulk segments)

    // row buffers (short scans: one block, RowBlock), debug dumps, and the kernel arguments that every launch of the call starts from
    int reserve(int64_t c0, int64_t c1) {
        const size_t N = size_t(shape.n);
        const bool rip = shape.rip;
        const RowBlock& blk = sched.block;
        if (sched.packed_rows) {
            HIPC(c, c->o_block.reserve(blk.words));
            HIPC(c, c->h_block.reserve(blk.words * 8, blk.words * 8 + blk.words));
        } else {
            HIPC(c, c->o_seq.reserve(N)); HIPC(c, c->o_start.reserve(N)); HIPC(c, c->o_stop.reserve(N));
            HIPC(c, c->o_status.reserve(N)); HIPC(c, c->o_kld.reserve(N)); HIPC(c, c->o_gc.reserve(N));
            if (rip) { HIPC(c, c->o_pi.reserve(N)); HIPC(c, c->o_si.reserve(N)); HIPC(c, c->o_cri.reserve(N)); }
        }
        HIPC(c, c->o_sw.reserve(N)); HIPC(c, c->o_sg.reserve(N));
        if (dbg_counts) {
            HIPC(c, c->o_counts.reserve(N * size_t(c->nprof)));
            HIPC(c, hipMemsetAsync(c->o_counts.p, 0, N * size_t(c->nprof) * 4, c->stream));
        }
        if (dbg_meta) {
            HIPC(c, c->o_meta.reserve(N * 3));
            HIPC(c, hipMemsetAsync(c->o_meta.p, 0, N * 3 * 8, c->stream));
        }
        P.codes = c->b().d_codes.p; P.inv = c->b().d_inv.p; P.low = c->b().d_low.p;
        P.descs = c->d_desc.p; P.ig = c->d_ig.p; P.log_tab = c->d_logtab.p; P.log_tab64 = c->d_logtab64.p; P.log_tab32 = c->d_logtab32.p;
        P.n_desc = c->b().n_seq + 1;
        P.kmin = c->kmin; P.kmax = c->kmax; P.w = shape.w; P.inc = shape.inc; P.flags = shape.flags; P.c0 = c0; P.c1 = c1;
        P.orphan_cap = sched.orphan_cap; P.lv = sched.lv; P.chunk = sched.chunk;
        P.nprof = int32_t(c->nprof);
        if (sched.packed_rows) {
            double* b = c->o_block.p;
            P.start = reinterpret_cast<int64_t*>(b + blk.start); P.stop = reinterpret_cast<int64_t*>(b + blk.stop);
            P.kld = b + blk.kld; P.gc = b + blk.gc;
            P.pi = rip ? b + blk.pi : nullptr; P.si = rip ? b + blk.si : nullptr; P.cri = rip ? b + blk.cri : nullptr;
            P.seq_index = reinterpret_cast<int32_t*>(b + blk.seq_index); P.status = reinterpret_cast<uint32_t*>(b + blk.status);
        } else {
            P.seq_index = c->o_seq.p; P.start = c->o_start.p; P.stop = c->o_stop.p; P.status = c->o_status.p;
            P.kld = c->o_kld.p; P.gc = c->o_gc.p;
            P.pi = rip ? c->o_pi.p : nullptr; P.si = rip ? c->o_si.p : nullptr; P.cri = rip ? c->o_cri.p : nullptr;
        }
        P.sw = c->o_sw.p; P.sg = c->o_sg.p;
        P.dbg_counts = dbg_counts ? c->o_counts.p : nullptr;
        P.dbg_meta = dbg_meta ? c->o_meta.p : nullptr;
        P.dbg_ivom = nullptr;
        if (c->want_ivom) {
            HIPC(c, c->o_ivom.reserve(N * 2 * nk));
            HIPC(c, hipMemsetAsync(c->o_ivom.p, 0, N * 2 * nk * sizeof(double), c->stream));
            P.dbg_ivom = c->o_ivom.p;
        }
        P.unused_stamps = nullptr;
        P.rc_tab = c->d_rctab.p; P.in_list = nullptr; P.in_count = nullptr; P.out_list = nullptr; P.out_count = nullptr;
        P.sel_mode = 0; P.sel_mod = sched.sel_mod; P.queue = nullptr; P.queue_n = 1; P.slide_pp = sched.slide_pp; P.ig_ring = nullptr;
        P.verdict = nullptr; P.my_form = 0u;
        return FRISK_OK;
    }

    // the 16-bit form (scan_kernel.h) over the candidates that PP names
    hipError_t launch16(const ScanParams& PP, int g, hipStream_t st) const {
        return launch_scan16_form(sched.form16, PP, sched.lds_total, g, st);
    }

    // rows [r0, r1) to the caller's buffers
    int copy_rows(int64_t r0, int64_t r1, hipStream_t st) {
        const size_t m = size_t(r1 - r0);
        if (sched.packed_rows) {        // (always the whole scan: short scans run in one segment) - unpacked behind the final wait
            HIPC(c, hipMemcpyAsync(c->h_block.p, c->o_block.p, sched.block.words * 8, hipMemcpyDeviceToHost, st));
            return FRISK_OK;
        }
        HIPC(c, hipMemcpyAsync(seq_index + r0, P.seq_index + r0, m * 4, hipMemcpyDeviceToHost, st));
        HIPC(c, hipMemcpyAsync(start + r0, P.start + r0, m * 8, hipMemcpyDeviceToHost, st));
        HIPC(c, hipMemcpyAsync(stop + r0, P.stop + r0, m * 8, hipMemcpyDeviceToHost, st));
        HIPC(c, hipMemcpyAsync(status + r0, P.status + r0, m * 4, hipMemcpyDeviceToHost, st));
        HIPC(c, hipMemcpyAsync(kld + r0, P.kld + r0, m * 8, hipMemcpyDeviceToHost, st));
        HIPC(c, hipMemcpyAsync(gc + r0, P.gc + r0, m * 8, hipMemcpyDeviceToHost, st));
        if (shape.rip) {
            HIPC(c, hipMemcpyAsync(pi + r0, P.pi + r0, m * 8, hipMemcpyDeviceToHost, st));
            HIPC(c, hipMemcpyAsync(si + r0, P.si + r0, m * 8, hipMemcpyDeviceToHost, st));
            HIPC(c, hipMemcpyAsync(cri + r0, P.cri + r0, m * 8, hipMemcpyDeviceToHost, st));
        }
        return FRISK_OK;
    }

    // every path but the narrow-counter one: one launch over the whole range, the rows' scalar tail, the rows to the host
    int enqueue_whole() {
        const int64_t n = shape.n;
        hipError_t e = hipSuccess;
        if (sched.path == SCAN_PATH_BIG) {      // 32-bit tables of all orders in a global scratch slice per workgroup
            const int64_t stride = (c->nprof + 3) / 4 * 4;
            HIPC(c, c->d_big.reserve(size_t(sched.big_grid) * size_t(stride)));
            HIPC(c, hipMemsetAsync(c->d_big.p, 0, size_t(sched.big_grid) * size_t(stride) * 4, c->stream));
            e = launch_scan_big(P, shape.debug, sched.big_grid, c->d_big.p, stride, c->stream);
        } else {        // (one or two workgroups per CU: the form says)
            e = launch16(P, sched.grid, c->stream);
        }
        HIPC(c, e);
        if (sched.path != SCAN_PATH_BIG) {      // the LDS kernels leave the rows' scalar tail to one thread per row
            HIPC(c, launch_finish_rows(grid_for(n, 256, 1 << 20), c->stream, n, P.status, P.kld, P.gc, P.sw, P.sg));
        }
        HIPC(c, hipEventRecord(c->ev1, c->stream));
        return copy_rows(0, n, c->stream);
    }

    // The sample of the adaptive width, and its own hand-overs (list 1 -> 8-bit -> list 2 -> 16-bit) now, so that lists and counters
    // are free for the bulk segments and no later pass touches rows of another segment
    int sample() {
        const int64_t n = shape.n, nsample = sched.nsample, chunk8 = sched.chunk8;
        ScanParams S = P;
        S.chunk = int32_t(chunk8);
        unsigned int* cnt = c->d_ovf_count.p;       // (the sample counts where segment 0 will)
        S.sel_mode = 1; S.out_list = c->d_ovf_list.p; S.out_count = cnt + SCAN_CNT_LIST1;
        if (sched.dealt) { S.queue = cnt + SCAN_CNT_BULK_QUEUES; S.queue_n = SCAN_CNT_BULK_QUEUE_N; }
        HIPC(c, launch_scan8_form(sched.form_sample, S, c->num_cu, nsample, c->stream));
        // The verdict is taken ON THE DEVICE (scan8_decide_kernel, one thread behind the sample): the host queues all three bulk forms
        // behind it, each with the verdict's address and its own number, and two of them return at once - no host synchronisation
        // in the first scan of a batch (round 3: sample -> copy -> hipStreamSynchronize -> decide -> launch).  The rule:
        // 4-bit pays while fewer than about three windows in ten have to be redone (round 3, bench shard with simple repeats at
        // 0.05 / 0.1 / 0.2 / 0.3 per kb = 10 / 20 / 37 / 51 % of the scored windows handed on: 4-bit bulk 7.27 / 7.96 / 8.97 /
        // 9.98 ms, 8-bit bulk 8.51 / 8.57 / 8.71 / 8.78 ms - tools/exp/width_sweep.sh); the side table pays when the plain form
        // would hand on more than FRISK_SIDE_SHARE of the windows that are scored (it costs a scored window 1.0 ns - ten
        // instructions per position: 6.97 against 6.59 ms per scan -, a window handed on 18 ns: tools/exp/side_rate.py)
        HIPC(c, launch_scan8_decide(cnt, static_cast<unsigned int>(nsample * chunk8), sched.narrow8 && !shape.debug ? 1 : 0,
                                    c->d_verdict.p, c->stream));
        ScanParams H = P;
        H.in_list = c->d_ovf_list.p; H.in_count = cnt + SCAN_CNT_LIST1;
        H.out_list = c->d_ovf_list2.p; H.out_count = cnt + SCAN_CNT_LIST2;
        if (sched.dealt) H.queue = cnt + SCAN_CNT_QUEUE8;
        HIPC(c, launch_scan8_form(sched.form_handover, H, c->num_cu, nsample * chunk8, c->stream));
        ScanParams H2 = P;
        H2.in_list = c->d_ovf_list2.p; H2.in_count = cnt + SCAN_CNT_LIST2;
        int g16 = int(std::min<int64_t>(n, int64_t(c->num_cu)));
        if (g16 >= 8) g16 &= ~7;
        HIPC(c, launch16(H2, g16, c->stream));
        static_assert(SCAN_CNT_LIST1 == 0 && SCAN_CNT_LIST2 == 1, "the two list lengths lead the block: one copy brings both");
        HIPC(c, hipMemcpyAsync(novf_sample, cnt, sizeof(novf_sample), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemsetAsync(cnt, 0, SCAN_CNT_TOTAL * sizeof(unsigned int), c->stream));
        return FRISK_OK;
    }

    // Rows [r0, r1) of this scan on stream `st`: bulk launch, the two hand-over launches and the rows' scalar tail.  Segment `seg`
    // has its own slice of the two lists (from entry r0) and its own counters (ScanCounter, scan_params.h).  Which kernel a launch
    // runs is the schedule's statement (sched.form_*).
    int run_rows(int seg, int64_t r0, int64_t r1, hipStream_t st, bool fork_tail) {
        const int64_t m = r1 - r0, chunk8 = sched.chunk8;
        ScanParams R = P;
        R.c0 = P.c0 + r0; R.c1 = P.c0 + r1;
        R.seq_index += r0; R.start += r0; R.stop += r0; R.status += r0; R.kld += r0; R.gc += r0; R.sw += r0; R.sg += r0;
        if (shape.rip) { R.pi += r0; R.si += r0; R.cri += r0; }
        if (R.dbg_counts) R.dbg_counts += r0 * int64_t(c->nprof);
        if (R.dbg_meta) R.dbg_meta += r0 * 3;
        if (R.dbg_ivom) R.dbg_ivom += r0 * 2 * int64_t(nk);
        unsigned int* cnt = c->d_ovf_count.p + SCAN_CNT_SEGMENT * seg;
        int64_t* list1 = c->d_ovf_list.p + r0;
        int64_t* list2 = c->d_ovf_list2.p + r0;
        ScanParams B = R;                       // the bulk launch
        B.chunk = int32_t(chunk8);
        B.sel_mode = sched.sel_mode;
        if (sched.bulk == 4) { B.out_list = list1; B.out_count = cnt + SCAN_CNT_LIST1; }
        else { B.out_list = list2; B.out_count = cnt + SCAN_CNT_LIST2; }
        if (sched.dealt) { B.queue = cnt + SCAN_CNT_BULK_QUEUES; B.queue_n = SCAN_CNT_BULK_QUEUE_N; }
        const int64_t mchunks = (m + chunk8 - 1) / chunk8;
        const int64_t bulk_chunks = sched.sel_mode == 2 ? mchunks - (mchunks + B.sel_mod - 1) / B.sel_mod : mchunks;
        if (sched.sample) {                     // plain 4-bit / 4-bit + side table / 8-bit: the device's verdict lets one of them run
            B.verdict = c->d_verdict.p;
            B.out_list = list1; B.out_count = cnt + SCAN_CNT_LIST1;
            B.my_form = 1u;
            HIPC(c, launch_scan8_form(sched.form_verdict[0], B, c->num_cu, bulk_chunks, st));
            B.my_form = 2u;
            HIPC(c, launch_scan8_form(sched.form_verdict[1], B, c->num_cu, bulk_chunks, st));
            B.my_form = 3u;
            B.out_list = list2; B.out_count = cnt + SCAN_CNT_LIST2;
            HIPC(c, launch_scan8_form(sched.form_verdict[2], B, c->num_cu, bulk_chunks, st));
        } else
        HIPC(c, launch_scan8_form(sched.form_bulk, B, c->num_cu, bulk_chunks, st));
        if (sched.bulk == 4) {                  // list 1 (4-bit hand-overs) -> 8-bit -> list 2
            ScanParams H = R;
            H.in_list = list1; H.in_count = cnt + SCAN_CNT_LIST1;
            H.out_list = list2; H.out_count = cnt + SCAN_CNT_LIST2;
            if (sched.dealt) H.queue = cnt + SCAN_CNT_QUEUE8;
            HIPC(c, launch_scan8_form(sched.form_handover, H, c->num_cu, m, st));
        }
        // list 2 -> 16-bit counters, one window per workgroup at a time (a no-op when the list is empty)
        R.in_list = list2; R.in_count = cnt + SCAN_CNT_LIST2;
        int g16 = int(std::min<int64_t>(m, int64_t(c->num_cu)));
        if (g16 >= 8) g16 &= ~7;
        HIPC(c, launch16(R, g16, st));
        if (fork_tail) {        // the tail segment starts here: beside this segment's scalar tail and its rows' way to the host
            HIPC(c, hipEventRecord(c->ev_fork, st));
            HIPC(c, hipStreamWaitEvent(c->tail_stream, c->ev_fork, 0));
        }
        HIPC(c, launch_finish_rows(grid_for(m, 256, 1 << 20), st, m, R.status, R.kld, R.gc, R.sw, R.sg));
        return FRISK_OK;
    }

    // the narrow-counter path (scan8_kernel.h): lists, counters and ring, the sample, then the rows in one or two segments
    int enqueue_narrow() {
        const int64_t n = shape.n, cut = sched.cut;
        HIPC(c, c->d_ovf_list.reserve(size_t(n)));
        HIPC(c, c->d_ovf_list2.reserve(size_t(n)));
        HIPC(c, hipMemsetAsync(c->d_ovf_count.p, 0, SCAN_CNT_TOTAL * sizeof(unsigned int), c->stream));
        if (sched.ring_slices > 0) {    // a copy of the genome table (one base address for both), then one slice per workgroup launched
            const double* had = c->d_ig_ring.p;
            HIPC(c, c->d_ig_ring.reserve(nk + size_t(sched.ring_slices) * (20 * FRISK8_RING_COLS + FRISK8_RING_PAD)));
            if (c->d_ig_ring.p != had || c->ring_gen != c->ig_gen) {        // (once per genome table, not once per scan)
                HIPC(c, hipMemcpyAsync(c->d_ig_ring.p, c->d_ig.p, nk * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
                c->ring_gen = c->ig_gen;
            }
            P.ig_ring = c->d_ig_ring.p;
        }
        if (sched.sample) { if (int rc = sample()) return rc; }
        if (int rc = run_rows(0, 0, cut, c->stream, cut < n)) return rc;
        if (cut < n) {
            if (int rc = run_rows(1, cut, n, c->tail_stream, false)) return rc;
            HIPC(c, hipEventRecord(c->ev_tail_kernels, c->tail_stream));
            if (int rc = copy_rows(cut, n, c->tail_stream)) return rc;
            HIPC(c, hipEventRecord(c->ev_tail_done, c->tail_stream));
            if (int rc = copy_rows(0, cut, c->stream)) return rc;
            HIPC(c, hipStreamWaitEvent(c->stream, c->ev_tail_kernels, 0));
            HIPC(c, hipEventRecord(c->ev1, c->stream));                     // every scan kernel of this call has finished
            HIPC(c, hipStreamWaitEvent(c->stream, c->ev_tail_done, 0));
            return FRISK_OK;
        }
        HIPC(c, hipEventRecord(c->ev1, c->stream));
        return copy_rows(0, n, c->stream);
    }

    int enqueue() {
        HIPC(c, hipEventRecord(c->ev0, c->stream));
        return sched.path == SCAN_PATH_NARROW ? enqueue_narrow() : enqueue_whole();
    }

    // debug dumps and counters to the host, the one wait of the call, then what the host does with the rows
    int collect() {
        const size_t N = size_t(shape.n);
        unsigned int novf[SCAN_CNT_SEGMENT + SCAN_CNT_LIST2 + 1] = {0}, verdict_host[4] = {0, 0, 0, 0};
        if (dbg_counts)
            HIPC(c, hipMemcpyAsync(dbg_counts, c->o_counts.p, N * size_t(c->nprof) * 4, hipMemcpyDeviceToHost, c->stream));
        if (dbg_meta) HIPC(c, hipMemcpyAsync(dbg_meta, c->o_meta.p, N * 3 * 8, hipMemcpyDeviceToHost, c->stream));
        if (c->want_ivom) HIPC(c, hipMemcpyAsync(c->want_ivom, c->o_ivom.p, N * 2 * nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (sched.path == SCAN_PATH_NARROW) HIPC(c, hipMemcpyAsync(novf, c->d_ovf_count.p, sizeof(novf), hipMemcpyDeviceToHost, c->stream));
        if (sched.sample) HIPC(c, hipMemcpyAsync(verdict_host, c->d_verdict.p, sizeof(verdict_host), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        c->scan_stat[0] = sched.bulk; c->scan_stat[3] = sched.segments; c->scan_stat[4] = sched.side ? 1 : 0;
        if (sched.sample) {             // what the device decided: remembered per batch and geometry (later scans launch that form alone)
            frisk_ctx::Batch& VB = c->b();
            VB.width_hint = verdict_host[0] == 3u ? 8 : 4; VB.hint_w = shape.w; VB.hint_inc = shape.inc; VB.hint_side = verdict_host[0] == 2u ? 1 : 0;
            c->scan_stat[0] = VB.width_hint;
            c->scan_stat[4] = VB.hint_side;
        }
        if (sched.packed_rows) {
            const double* b = reinterpret_cast<const double*>(c->h_block.p);
            const RowBlock& blk = sched.block;
            std::memcpy(start, b + blk.start, N * 8); std::memcpy(stop, b + blk.stop, N * 8);
            std::memcpy(kld, b + blk.kld, N * 8); std::memcpy(gc, b + blk.gc, N * 8);
            if (shape.rip) { std::memcpy(pi, b + blk.pi, N * 8); std::memcpy(si, b + blk.si, N * 8); std::memcpy(cri, b + blk.cri, N * 8); }
            std::memcpy(seq_index, b + blk.seq_index, N * 4); std::memcpy(status, b + blk.status, N * 4);
        }
        c->scan_stat[5] = sched.kmin1_form && c->scan_stat[0] == 4 ? 1 : 0;
        c->scan_stat[1] = novf[SCAN_CNT_LIST1] + novf[SCAN_CNT_SEGMENT + SCAN_CNT_LIST1] + novf_sample[0];
        c->scan_stat[2] = novf[SCAN_CNT_LIST2] + novf[SCAN_CNT_SEGMENT + SCAN_CNT_LIST2] + novf_sample[1];
        if (c->b().tiled)               // descriptor index -> index of the scaffold in the FASTA
            for (size_t r = 0; r < N; ++r) seq_index[r] = c->b().tiles[size_t(seq_index[r])].scaf;
        float ms = 0;
        HIPC(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->ms[0] = ms;
        return FRISK_OK;
    }
};

// frisk_scan in five steps: validate the call, decide the schedule (plan_scan_schedule, scan_schedule.h), reserve the buffers,
// enqueue the launches and copies, collect the rows
int scan_impl(frisk_ctx* c, int32_t w, int32_t inc, uint32_t flags, int64_t c0, int64_t c1, int64_t cap,
              int32_t* seq_index, int64_t* start, int64_t* stop, uint32_t* status, double* kld, double* gc,
              double* pi, double* si, double* cri, uint32_t* dbg_counts, int64_t* dbg_meta) {
    if (!c) return FRISK_E_ARG;
    if (!c->profile_final) return fail(c, FRISK_E_STATE, "frisk_scan: genome profile not finalised");
    int64_t ncand_all = 0;
    int rc = frisk_scan_plan(c, w, inc, flags, &ncand_all);
    if (rc) return rc;
    if (c1 < 0) c1 = ncand_all;
    if (c0 < 0 || c0 > c1 || c1 > ncand_all) return fail(c, FRISK_E_ARG, "candidate range outside [0, n_candidates]");
    const int64_t n = c1 - c0;
    if (cap < n) return fail(c, FRISK_E_CAP, "output capacity too small: need " + std::to_string(n));
    const bool rip = (flags & FRISK_SCAN_RIP) != 0;
    if (rip && !(c->kmin <= 2 && c->kmax >= 2))
        return fail(c, FRISK_E_ARG, "RIP indices need dinucleotide counts: kmin <= 2 <= kmax (reference L478)");
    if (rip && (!pi || !si || !cri)) return fail(c, FRISK_E_ARG, "FRISK_SCAN_RIP needs pi/si/cri buffers");
    if (!seq_index || !start || !stop || !status || !kld || !gc) return fail(c, FRISK_E_ARG, "null output buffer");
    c->ms[0] = 0.0;
    if (n == 0) return FRISK_OK;
    HIPC(c, hipSetDevice(c->device));
    if (int rs = settle_stream(c)) return rs;

    const ScanShape shape = scan_shape_of(c, n, w, inc, flags, dbg_counts || dbg_meta);
    const ScanSchedule sched = plan_scan_schedule(shape);
    if (sched.error) return fail(c, sched.error_code, sched.error);
    c->scan_stat[0] = 16; c->scan_stat[1] = 0; c->scan_stat[2] = 0; c->scan_stat[3] = 1; c->scan_stat[4] = 0; c->scan_stat[5] = 0;

    ScanRun run{c, shape, sched, seq_index, start, stop, status, kld, gc, pi, si, cri, dbg_counts, dbg_meta,
                ScanParams(), size_t(1) << (2 * c->kmax), {0, 0}};
    if ((rc = run.reserve(c0, c1))) return rc;
    if ((rc = run.enqueue())) return rc;
    return run.collect();
}

}  // namespace

int frisk_scan(frisk_ctx* c, int32_t w, int32_t inc, uint32_t flags, int64_t c0, int64_t c1, int64_t cap,
               int32_t* seq_index, int64_t* start, int64_t* stop, uint32_t* status, double* kld, double* gc,
               double* pi, double* si, double* cri, uint32_t* dbg_counts, int64_t* dbg_meta) {
    const int rc = scan_impl(c, w, inc, flags, c0, c1, cap, seq_index, start, stop, status, kld, gc, pi, si, cri, dbg_counts, dbg_meta);
    if (rc != FRISK_OK && c) {
        // a failure after work was queued: copies may still target the caller's row buffers (and locals of the call), kernels of
        // the tail segment may still run - nothing of this call is in flight once it has returned
        const std::string msg = c->err;
        if (hipSetDevice(c->device) == hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipStreamSynchronize(c->tail_stream);
            (void)hipGetLastError();
        }
        c->err = msg;
    }
    return rc;
}

int frisk_scan_ivom(frisk_ctx* c, int32_t w, int32_t inc, uint32_t flags, int64_t c0, int64_t c1, int64_t cap,
                    double* window_ivom, double* genome_ivom) {
    if (!c || !window_ivom || !genome_ivom) return FRISK_E_ARG;
    if (c->kmax > 6) return fail(c, FRISK_E_ARG, "frisk_scan_ivom: the per-max-mer dump exists for kmax <= 6 only");
    int64_t ncand = 0;
    int rc = frisk_scan_plan(c, w, inc, flags, &ncand);
    if (rc) return rc;
    if (c1 < 0) c1 = ncand;
    if (c0 < 0 || c0 > c1 || c1 > ncand) return fail(c, FRISK_E_ARG, "candidate range outside [0, n_candidates]");
    const int64_t n = c1 - c0;
    if (cap < n) return fail(c, FRISK_E_CAP, "output capacity too small: need " + std::to_string(n));
    if (c->plan_maxwin > 65535) return fail(c, FRISK_E_ARG, "frisk_scan_ivom: windows of at most 65535 bases");
    const size_t nk = size_t(1) << (2 * c->kmax), N = size_t(std::max<int64_t>(n, 1));
    std::vector<double> raw(N * 2 * nk), kld(N), gc(N), pi(N), si(N), cri(N);
    std::vector<int32_t> seq(N);
    std::vector<int64_t> start(N), stop(N), meta(N * 3);
    std::vector<uint32_t> status(N);
    c->want_ivom = raw.data();
    rc = frisk_scan(c, w, inc, flags & ~FRISK_SCAN_RIP, c0, c1, int64_t(N), seq.data(), start.data(), stop.data(), status.data(),
                    kld.data(), gc.data(), nullptr, nullptr, nullptr, nullptr, meta.data());
    c->want_ivom = nullptr;
    if (rc) return rc;
    for (int64_t r = 0; r < n; ++r) {           // normalise over the window's present max-mers (L450-454), in index order
        const double* iw = raw.data() + size_t(r) * 2 * nk;
        const double* ig = iw + nk;
        // compensated (Neumaier) sums: a plain running sum over a window's ~10^3 max-mers loses up to that many ulps of Sw, Sg,
        // which shifts every normalised entry alike (measured: 87 ulps at K = 6); the scan kernels sum these exactly
        double sw = 0.0, sg = 0.0, cw = 0.0, cg = 0.0;
        auto add = [](double& s, double& comp, double v) {
            const double t = s + v;
            comp += std::fabs(s) >= std::fabs(v) ? (s - t) + v : (v - t) + s;
            s = t;
        };
        for (size_t k = 0; k < nk; ++k) { add(sw, cw, iw[k]); add(sg, cg, ig[k]); }
        sw += cw;
        sg += cg;
        for (size_t k = 0; k < nk; ++k) {
            window_ivom[size_t(r) * nk + k] = iw[k] != 0.0 ? iw[k] / sw : 0.0;
            genome_ivom[size_t(r) * nk + k] = iw[k] != 0.0 ? ig[k] / sg : 0.0;
        }
    }
    return FRISK_OK;
}

char* frisk_format_rows(int64_t n, const char* const* names, const int32_t* seq_index, const int64_t* start, const int64_t* stop,
                        const uint8_t* kld_is_int0, const double* kld, const double* gc, const double* pi, const double* si,
                        const double* cri, int64_t* out_len) {
    if (out_len) *out_len = 0;
    if (n < 0 || (n > 0 && (!names || !seq_index || !start || !stop || !kld || !gc))) return nullptr;
    if ((pi || si || cri) && !(pi && si && cri)) return nullptr;
    frisk_text::Columns c{n, names, seq_index, start, stop, kld_is_int0, kld, gc, pi, si, cri};
    return frisk_text::format_all(c, out_len);
}
void frisk_free(void* p) { std::free(p); }
int64_t frisk_last_scan_stat(const frisk_ctx* c, int which) { return (c && which >= 0 && which < 6) ? c->scan_stat[which] : -1; }

}  // extern "C"
