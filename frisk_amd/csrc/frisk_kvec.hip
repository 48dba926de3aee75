// frisk_kvec.hip - frisk_window_vectors of the C ABI (include/frisk_hip.h): the projection's k-mer proportion vectors of arbitrary
// ranges of the resident batch, counted, folded and divided on the device (kvec_kernels.h), batch of rows by batch of rows.  The
// context is frisk_ctx.h's.  gfx950 (MI355X) only.  Build: see __graft_entry__.build_hip().
#include <algorithm>
#include <string>
#include <vector>

#include "frisk_ctx.h"
#include "kvec_kernels.h"

namespace {

constexpr size_t KVEC_X_BYTES = size_t(256) << 20;      // the device-side block of X at batch_rows = 0

// the kept codes of every order (c <= revcomp(c), canonical order) as pairs of counter indices (c, rc(c)) in profile layout a..b
KvecShape kvec_shape(int a, int b, std::vector<uint32_t>& pairs) {
    KvecShape s{};
    s.a = a; s.b = b;
    s.nprof = int(table_offset(a, b + 1));
    pairs.clear();
    for (int x = a; x <= b; ++x) {
        s.feat0[x] = int(pairs.size() / 2);
        const uint32_t off = uint32_t(table_offset(a, x));
        for (uint32_t c = 0; c < (1u << (2 * x)); ++c) {
            const uint32_t rc = revcomp_code(c, x);
            if (c <= rc) { pairs.push_back(off + c); pairs.push_back(off + rc); }
        }
    }
    s.feat0[b + 1] = int(pairs.size() / 2);
    return s;
}

}  // namespace

extern "C" int frisk_window_vectors(frisk_ctx* c, const int32_t* seq_index, const int64_t* start, const int64_t* stop, int64_t n, int kmin,
                                    int kmax, int64_t batch_rows, double* X, int64_t* nn, uint32_t* status) {
    if (!c) return FRISK_E_ARG;
    if (kmin < 1 || kmin > kmax || kmax > FRISK_KVEC_MAX_K) return fail(c, FRISK_E_ARG, "frisk_window_vectors: orders must satisfy 1 <= kmin <= kmax <= 7");
    if (n < 0 || batch_rows < 0) return fail(c, FRISK_E_ARG, "frisk_window_vectors: n < 0 or batch_rows < 0");
    const frisk_ctx::Batch& B = c->b();
    if (!B.have_seq) return fail(c, FRISK_E_ARG, "frisk_window_vectors: no resident sequence batch");
    if (B.tiled) return fail(c, FRISK_E_ARG, "frisk_window_vectors: the resident batch holds tiles, not whole scaffolds");
    if (n == 0) return FRISK_OK;
    if (!seq_index || !start || !stop || !X || !nn || !status) return fail(c, FRISK_E_ARG, "frisk_window_vectors: null array");
    std::vector<int64_t> ranges(size_t(n) * 2);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t s = seq_index[r];
        if (s < 0 || s >= B.n_seq) return fail(c, FRISK_E_ARG, "frisk_window_vectors: sequence index out of range in row " + std::to_string(r));
        if (start[r] < 0 || stop[r] <= start[r] || stop[r] > B.seq_len[size_t(s)] || stop[r] - start[r] > int64_t(0xFFFFFFFFll))
            return fail(c, FRISK_E_ARG, "frisk_window_vectors: range outside the scaffold (or empty, or of 2^32 bases or more) in row " + std::to_string(r));
        ranges[size_t(2 * r)] = B.seq_off[size_t(s)] + start[r];
        ranges[size_t(2 * r + 1)] = stop[r] - start[r];
    }
    HIPC(c, hipSetDevice(c->device));
    if (int rc = settle_stream(c)) return rc;
    std::vector<uint32_t> pairs;
    const KvecShape shape = kvec_shape(kmin, kmax, pairs);
    const int64_t F = shape.feat0[kmax + 1];
    const int64_t rows = std::min<int64_t>(n, batch_rows ? batch_rows : std::max<int64_t>(1, int64_t(KVEC_X_BYTES / (size_t(F) * sizeof(double)))));
    DevBuf<int64_t> d_ranges, d_nn;             // (freed on every return below)
    DevBuf<uint32_t> d_pairs, d_status;
    DevBuf<double> d_X;
    HIPC(c, d_ranges.reserve(ranges.size(), ranges.size()));
    HIPC(c, d_nn.reserve(size_t(n), size_t(n)));
    HIPC(c, d_status.reserve(size_t(n), size_t(n)));
    HIPC(c, d_pairs.reserve(pairs.size(), pairs.size()));
    HIPC(c, d_X.reserve(size_t(rows) * size_t(F), size_t(rows) * size_t(F)));
    HIPC(c, hipMemcpyAsync(d_ranges.p, ranges.data(), ranges.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(d_pairs.p, pairs.data(), pairs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const size_t lds = size_t(shape.nprof) * sizeof(uint32_t);          // 87 376 B at 1..7: above the 64 KB a launch gets unasked
    HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kvec_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    double kernel_ms = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
        const int64_t m = std::min(rows, n - r0);
        HIPC(c, hipEventRecord(c->ev0, c->stream));
        kvec_kernel<<<grid_for(m, 1, FRISK_KVEC_GRID_CAP), FRISK_KVEC_THREADS, lds, c->stream>>>(
            B.d_codes.p, B.d_inv.p, B.d_low.p, d_ranges.p + 2 * r0, m, shape, d_pairs.p, d_X.p, d_nn.p + r0, d_status.p + r0);
        HIPC(c, hipGetLastError());
        HIPC(c, hipEventRecord(c->ev1, c->stream));
        // (in stream order: the next batch's kernel overwrites d_X only after this copy has read it)
        HIPC(c, hipMemcpyAsync(X + r0 * F, d_X.p, size_t(m) * size_t(F) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        HIPC(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        kernel_ms += ms;
    }
    HIPC(c, hipMemcpyAsync(nn, d_nn.p, size_t(n) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(status, d_status.p, size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->ms[3] = kernel_ms;
    return FRISK_OK;
}
