// ipca_kernels.h - incremental PCA (sklearn's IncrementalPCA.partial_fit, the reference's L1629-1631), FP64 on the device.
//
// The state (rows seen, column mean and variance, singular values S and components V) stays on the device between batches.
// One batch of b rows goes through
//   statistics   column sums of the batch (colsum_part + ipca_colsum), then sum(x - T) and sum (x - T)^2 per column with
//                T the batch mean (ipca_dev_part), then sklearn's _incremental_mean_and_var merge, operation for operation,
//                one thread per column (ipca_merge);
//   stack        the zero-padded A: first batch the batch minus the new mean; later batches the d rows S_i V_i, the batch minus
//                its own mean, and the row sqrt(seen / total * b) (old mean - batch mean) (ipca_stack);
//   Gram         G = AT A through proj_cov_part / proj_cov_reduce (denom 1): exactly symmetric.
// The right singular vectors of A are the eigenvectors of G and S^2 its eigenvalues; the caller decomposes G and hands S and V
// back (commit), which also installs the batch's mean, variance and row count.
// Every reduction has a fixed order that depends on the shape only, and there is no floating-point atomic: every output is
// bit-identical from run to run.  Included from frisk_analysis.hip; it launches PCA's centring, covariance and transform kernels
// (proj_kernels.h) and the column sums of analysis_common.h over PCA's ranges.
#pragma once

#include "analysis_common.h"
#include "proj_kernels.h"

namespace frisk_ipca_impl {

using frisk_common::Buf;
using frisk_common::round_up;
using frisk_common::RowSplits;
using frisk_proj::COV_KSTEP;
using frisk_proj::COV_T;
using frisk_proj::MEAN_SPLITS;
using frisk_proj::MEAN_UNROLL;

// sum[c] = the split partials of column c in split order; T[c] = sum[c] / b (numpy's mean: the sum divided by the count)
__global__ __launch_bounds__(256) void ipca_colsum(const double* __restrict__ part, int nsplit, int64_t b, int64_t f,
                                                   double* __restrict__ sum, double* __restrict__ T) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c >= f) return;
    double s = 0.0;
    for (int p = 0; p < nsplit; ++p) s += part[int64_t(p) * f + c];
    sum[c] = s;
    T[c] = s / double(b);
}

// part[s][c] = sum of (X[r][c] - T[c]), part[nsplit + s][c] = sum of (X[r][c] - T[c])^2 over the rows r of split s, in row order
__global__ __launch_bounds__(256) void ipca_dev_part(const double* __restrict__ X, const double* __restrict__ T, int64_t b, int64_t f,
                                                     int64_t rows_per, int nsplit, double* __restrict__ part) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c >= f) return;
    const int64_t r0 = int64_t(blockIdx.y) * rows_per;
    const int64_t r1 = r0 + rows_per < b ? r0 + rows_per : b;
    const double t = T[c];
    double s1 = 0.0, s2 = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        const double e = X[r * f + c] - t;
        s1 += e;
        s2 += e * e;
    }
    part[int64_t(blockIdx.y) * f + c] = s1;
    part[(int64_t(nsplit) + blockIdx.y) * f + c] = s2;
}

// sklearn.utils.extmath._incremental_mean_and_var for one column (no NaN, no weights), in its order of operations:
// last = (mean, var, seen) of the rows before, new = this batch of b rows.
__global__ __launch_bounds__(256) void ipca_merge(const double* __restrict__ part, int nsplit, const double* __restrict__ new_sum_,
                                                  const double* __restrict__ last_mean, const double* __restrict__ last_var,
                                                  int64_t seen, int64_t b, int64_t f, double* __restrict__ mean_out,
                                                  double* __restrict__ var_out) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c >= f) return;
    double correction = 0.0, unnorm = 0.0;
    for (int p = 0; p < nsplit; ++p) {
        correction += part[int64_t(p) * f + c];
        unnorm += part[(int64_t(nsplit) + p) * f + c];
    }
    const double last_count = double(seen), new_count = double(b);
    const double new_sum = new_sum_[c];
    const double last_sum = seen ? last_mean[c] * last_count : 0.0;
    const double updated_count = last_count + new_count;
    mean_out[c] = (last_sum + new_sum) / updated_count;
    const double new_unnorm = unnorm - correction * correction / new_count;
    double updated = new_unnorm;                // the first batch (last_sample_count == 0)
    if (seen) {
        const double last_unnorm = last_var[c] * last_count;
        const double last_over_new = last_count / new_count;
        const double t = last_sum / last_over_new - new_sum;
        updated = last_unnorm + new_unnorm + last_over_new / updated_count * (t * t);
    }
    var_out[c] = updated / updated_count;
}

// A (rows_pad x f_pad, zero outside its rows x f).
// seen == 0: row r = X[r] - mean_new (r < b).
// seen > 0:  row i = S[i] Vt[i] (i < d); row d + r = X[r] - T (r < b); row d + b = coef (mean_old - T).
__global__ __launch_bounds__(256) void ipca_stack(const double* __restrict__ X, const double* __restrict__ T,
                                                  const double* __restrict__ mean_new, const double* __restrict__ mean_old,
                                                  const double* __restrict__ S, const double* __restrict__ Vt, int64_t seen, int64_t b,
                                                  int64_t f, int d, double coef, int64_t rows_pad, int64_t f_pad,
                                                  double* __restrict__ A) {
    const int64_t total = rows_pad * f_pad;
    const int64_t head = seen ? d : 0;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int64_t r = e / f_pad, c = e - r * f_pad;
        double v = 0.0;
        if (c < f) {
            if (r < head) v = S[r] * Vt[r * f + c];
            else if (r < head + b) v = X[(r - head) * f + c] - (seen ? T[c] : mean_new[c]);
            else if (seen && r == head + b) v = coef * (mean_old[c] - T[c]);
        }
        A[e] = v;
    }
}

constexpr int64_t TRANSFORM_PIECE = int64_t(1) << 23;       // doubles of padded rows per transform piece (64 MB)

// Device state of one incremental fit (the C handle frisk_ipca).
struct State {
    int device = 0;
    int64_t f = 0, f_pad = 0;
    int d = 0;
    int64_t seen = 0;                   // rows of the committed batches
    int64_t pending_b = 0;              // rows of the batch whose Gram matrix is out and not committed yet (0: none)
    bool fitted = false;                // S and V hold a committed decomposition
    frisk_common::DevMem mem;
    double *mean = nullptr, *var = nullptr, *mean_new = nullptr, *var_new = nullptr, *S = nullptr, *Vt = nullptr, *Vfd = nullptr;
    double *bsum = nullptr, *T = nullptr, *G = nullptr;
    Buf X, A, part, covpart, Y;
    frisk_common::EventTimer<4> timer;
    double ms[3] = {0.0, 0.0, 0.0};     // of the last gram(): upload, statistics + stack, Gram

    int create() {
        f_pad = round_up(f, COV_T);
        const size_t sf = size_t(f), sd = size_t(d);
        mean = mem.get<double>(sf); var = mem.get<double>(sf); mean_new = mem.get<double>(sf); var_new = mem.get<double>(sf);
        S = mem.get<double>(sd); Vt = mem.get<double>(sd * sf); Vfd = mem.get<double>(sd * sf);
        bsum = mem.get<double>(sf); T = mem.get<double>(sf); G = mem.get<double>(sf * sf);
        if (!mean || !var || !mean_new || !var_new || !S || !Vt || !Vfd || !bsum || !T || !G) return -2;
        return timer.create();
    }

    // Statistics, stack and Gram matrix of one batch; G_out[f * f].  Nothing of the committed state changes.  Returns 0 or -2.
    int gram(const double* X_in, int64_t b, double* G_out) {
        pending_b = 0;
        const int64_t rows = seen ? int64_t(d) + b + 1 : b;
        const int64_t rows_pad = round_up(rows, COV_KSTEP);
        const RowSplits sp(b, MEAN_SPLITS);
        const int64_t rows_per = sp.rows_per;
        const int nsplit = int(sp.count);
        const int Tn = int(f_pad / COV_T);
        const int ntile = Tn * (Tn + 1) / 2;
        const auto [ksplit, k_per] = frisk_proj::cov_ksplit(rows_pad, ntile);
        double* dX = X.ensure(size_t(b) * size_t(f));
        double* dA = A.ensure(size_t(rows_pad) * size_t(f_pad));
        double* dpart = part.ensure(2 * size_t(nsplit) * size_t(f));
        double* dcov = covpart.ensure(size_t(ksplit) * size_t(ntile) * COV_T * COV_T);
        if (!dX || !dA || !dpart || !dcov) return -2;
        FRISK_HIP_CHECK(timer.record(0));
        FRISK_HIP_CHECK(hipMemcpy(dX, X_in, size_t(b) * size_t(f) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(timer.record(1));
        const unsigned gf = unsigned((f + 255) / 256);
        hipLaunchKernelGGL(frisk_common::colsum_part<MEAN_UNROLL>, dim3(gf, unsigned(nsplit)), dim3(256), 0, 0, dX, b, f, rows_per, dpart);
        hipLaunchKernelGGL(ipca_colsum, dim3(gf), dim3(256), 0, 0, dpart, nsplit, b, f, bsum, T);
        hipLaunchKernelGGL(ipca_dev_part, dim3(gf, unsigned(nsplit)), dim3(256), 0, 0, dX, T, b, f, rows_per, nsplit, dpart);
        hipLaunchKernelGGL(ipca_merge, dim3(gf), dim3(256), 0, 0, dpart, nsplit, bsum, mean, var, seen, b, f, mean_new, var_new);
        const double coef = seen ? std::sqrt((double(seen) / double(seen + b)) * double(b)) : 0.0;
        const int64_t total = rows_pad * f_pad;
        const unsigned gs = unsigned(std::min<int64_t>((total + 255) / 256, 65536));
        hipLaunchKernelGGL(ipca_stack, dim3(gs), dim3(256), 0, 0, dX, T, mean_new, mean, S, Vt, seen, b, f, d, coef, rows_pad, f_pad,
                           dA);
        FRISK_HIP_CHECK(timer.record(2));
        hipLaunchKernelGGL(frisk_proj::proj_cov_part, dim3(unsigned(ntile), unsigned(ksplit)), dim3(256), 0, 0, dA, f_pad, rows_pad,
                           k_per, Tn, ntile, dcov);
        hipLaunchKernelGGL(frisk_proj::proj_cov_reduce, dim3(unsigned(ntile)), dim3(256), 0, 0, dcov, int(ksplit), Tn, ntile, f, 1.0, G);
        FRISK_HIP_CHECK(timer.record(3));
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipMemcpy(G_out, G, size_t(f) * size_t(f) * sizeof(double), hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k)
            if (timer.elapsed(k, k + 1, ms[k])) return -2;
        pending_b = b;
        return 0;
    }

    // S[d], Vt[d][f] (host) become the decomposition; Vfd is its transpose for the transform kernel.
    int upload_sv(const double* S_in, const double* Vt_in) {
        std::vector<double> vfd(size_t(f) * size_t(d));
        frisk_common::transpose(Vt_in, d, f, vfd.data());
        FRISK_HIP_CHECK(hipMemcpy(S, S_in, size_t(d) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(hipMemcpy(Vt, Vt_in, size_t(d) * size_t(f) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(hipMemcpy(Vfd, vfd.data(), vfd.size() * sizeof(double), hipMemcpyHostToDevice));
        return 0;
    }

    // The pending batch becomes part of the fit.  Returns 0 or -2.
    int commit(const double* S_in, const double* Vt_in) {
        if (int e = upload_sv(S_in, Vt_in)) return e;
        std::swap(mean, mean_new);
        std::swap(var, var_new);
        seen += pending_b;
        pending_b = 0;
        fitted = true;
        return 0;
    }

    int set(int64_t n_seen, const double* mean_in, const double* var_in, const double* S_in, const double* Vt_in) {
        pending_b = 0;
        seen = n_seen;
        fitted = n_seen > 0;
        if (!fitted) return 0;
        FRISK_HIP_CHECK(hipMemcpy(mean, mean_in, size_t(f) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(hipMemcpy(var, var_in, size_t(f) * sizeof(double), hipMemcpyHostToDevice));
        return upload_sv(S_in, Vt_in);
    }

    // Y_out[n][d] = (X - mean) V, in pieces of rows (each row's result does not depend on the piece it falls in).
    int transform(const double* X_in, int64_t n, double* Y_out) {
        const int64_t piece = std::max<int64_t>(1, std::min<int64_t>(n, TRANSFORM_PIECE / f_pad));
        double* dX = X.ensure(size_t(piece) * size_t(f));
        double* dA = A.ensure(size_t(piece) * size_t(f_pad));
        double* dY = Y.ensure(size_t(piece) * size_t(d));
        if (!dX || !dA || !dY) return -2;
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t m = std::min<int64_t>(piece, n - r0);
            FRISK_HIP_CHECK(hipMemcpy(dX, X_in + r0 * f, size_t(m) * size_t(f) * sizeof(double), hipMemcpyHostToDevice));
            const int64_t total = m * f_pad;
            const unsigned gc = unsigned(std::min<int64_t>((total + 255) / 256, 65536));
            hipLaunchKernelGGL(frisk_proj::proj_center, dim3(gc), dim3(256), 0, 0, dX, mean, m, f, m, f_pad, dA);
            hipLaunchKernelGGL(frisk_proj::proj_transform, dim3(unsigned((m + 3) / 4)), dim3(256), 0, 0, dA, Vfd, m, f, f_pad, d, dY);
            FRISK_HIP_CHECK(hipGetLastError());
            FRISK_HIP_CHECK(hipMemcpy(Y_out + r0 * d, dY, size_t(m) * size_t(d) * sizeof(double), hipMemcpyDeviceToHost));
        }
        return 0;
    }
};

}  // namespace frisk_ipca_impl

