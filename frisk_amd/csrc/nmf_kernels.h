// nmf_kernels.h - NMF as the reference's --runProjection NMF runs it (sklearn.decomposition.NMF(init=None, solver='cd',
// shuffle=False): sklearn/decomposition/_nmf.py _fit_coordinate_descent and _cdnmf_fast.pyx _update_cdnmf_fast), FP64.
//
// Layout (n rows, f features, d <= 16 components): X (n x f) stays on the device for the life of the handle; W is n x d; H is kept
// transposed, Ht f x d, as sklearn keeps it, so both coordinate-descent sweeps walk rows of d contiguous values.  Every reduction
// has a fixed order that depends on the shape only, and there is no floating-point atomic: every output is bit-identical from run
// to run.
//   Y = X Q   (n x p, p <= NMF_MAX_P)  one wave per R rows; lane l takes features l, l + 64, ... in order, then a wave butterfly.
//   Z = XT Q' (f x p)                  one lane per feature, the rows in `nsplit` contiguous splits, each in row order
//                                      (nmf_xtq_part); the splits summed in split order (nmf_xtq_reduce).
//   G = AT A  (d x d)                  one block per entry t <= r: thread i takes rows i, i + 256, ..., then block_sum; the entry
//                                      and its mirror are written from the same sum.
//   sweep                              _update_cdnmf_fast with the identity permutation: one lane per row, t = 0 .. d - 1 in
//                                      order, the gradient's sum over r in order; sum |projected gradient| per lane in t order,
//                                      block_sum per block, the blocks in index order by one thread (nmf_sum_parts).
// The two products serve the coordinate descent (p = d) and the range finder of the initialisation (p up to d + 10).  They are
// plain VALU: each is bound by reading X once (DESIGN.md section 9.4 has the measured fraction of the HBM rate).
// Included from frisk_analysis.hip before spectral_kernels.h; the C entry points there are thin wrappers of the driver below.  The
// sums, the row split, the width dispatch and the event timer are analysis_common.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "analysis_common.h"

namespace frisk_nmf_impl {

using frisk_common::block_sum;
using frisk_common::for_width;
using frisk_common::wave_sum;

constexpr int NMF_MAX_D = 16;       // components
constexpr int NMF_MAX_P = 26;       // columns of a product: d plus the range finder's 10 oversamples
constexpr int XTQ_SPLITS = 256;     // most row splits of XT Q'
constexpr int XTQ_MIN_ROWS = 32;    // fewest rows per split (but for the last)

// ---------------------------------------------------------------------------------------------------------- Y = X Q
// Wave w of block b owns rows (4 b + w) R .. + R - 1.
template <int PMAX, int R>
__global__ __launch_bounds__(256) void nmf_xq(const double* __restrict__ X, const double* __restrict__ Q, int64_t n, int64_t f, int p,
                                              double* __restrict__ Y) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * R;
    if (r0 >= n) return;                                    // the whole wave
    double acc[R][PMAX];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int q = 0; q < PMAX; ++q) acc[a][q] = 0.0;
    for (int64_t c = lane; c < f; c += 64) {
        double qv[PMAX];
#pragma unroll
        for (int q = 0; q < PMAX; ++q) qv[q] = q < p ? Q[c * p + q] : 0.0;
#pragma unroll
        for (int a = 0; a < R; ++a) {
            const double x = r0 + a < n ? X[(r0 + a) * f + c] : 0.0;
#pragma unroll
            for (int q = 0; q < PMAX; ++q) acc[a][q] += x * qv[q];
        }
    }
#pragma unroll
    for (int a = 0; a < R; ++a) {
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            if (r0 + a < n && q < p) {                      // uniform over the wave
                const double s = wave_sum(acc[a][q]);
                if (lane == 0) Y[(r0 + a) * p + q] = s;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- Z = XT Q'
// part[s][c][q] = sum over the rows r of split s, in order, of X[r][c] Q'[r][q].  Block (bx, s): features 64 bx .. 64 bx + 63.
template <int PMAX>
__global__ __launch_bounds__(64) void nmf_xtq_part(const double* __restrict__ X, const double* __restrict__ Q, int64_t n, int64_t f,
                                                   int p, int64_t rows_per, double* __restrict__ part) {
    const int64_t c = int64_t(blockIdx.x) * 64 + threadIdx.x;
    if (c >= f) return;
    const int64_t r0 = int64_t(blockIdx.y) * rows_per;
    const int64_t r1 = r0 + rows_per < n ? r0 + rows_per : n;
    double acc[PMAX];
#pragma unroll
    for (int q = 0; q < PMAX; ++q) acc[q] = 0.0;
#pragma unroll 4
    for (int64_t r = r0; r < r1; ++r) {
        const double x = X[r * f + c];
#pragma unroll
        for (int q = 0; q < PMAX; ++q)
            if (q < p) acc[q] += x * Q[r * p + q];
    }
    double* out = part + (int64_t(blockIdx.y) * f + c) * p;
#pragma unroll
    for (int q = 0; q < PMAX; ++q)
        if (q < p) out[q] = acc[q];
}

// Z[e] = the split partials of entry e (of f p) in split order
__global__ __launch_bounds__(256) void nmf_xtq_reduce(const double* __restrict__ part, int nsplit, int64_t total, double* __restrict__ Z) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= total) return;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += part[int64_t(k) * total + e];
    Z[e] = s;
}

// ---------------------------------------------------------------------------------------------------------- G = AT A
// A: m x d.  Block t d + r with t <= r computes G[t][r] and writes G[r][t] from the same sum.
__global__ __launch_bounds__(256) void nmf_gram(const double* __restrict__ A, int64_t m, int d, double* __restrict__ G) {
    __shared__ double red[4];
    const int t = int(blockIdx.x) / d, r = int(blockIdx.x) % d;
    if (t > r) return;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) s += A[i * d + t] * A[i * d + r];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        G[t * d + r] = s;
        G[r * d + t] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------- one sweep
// _update_cdnmf_fast(W, HHt, XHt, permutation = identity) on the m rows of W (m x d); part[b] = the block's sum of |pg|.
template <int DMAX>
__global__ __launch_bounds__(256) void nmf_sweep(double* __restrict__ W, const double* __restrict__ HHt, const double* __restrict__ XHt,
                                                 int64_t m, int d, double* __restrict__ part) {
    __shared__ double hh[DMAX * DMAX];
    __shared__ double red[4];
    for (int e = threadIdx.x; e < DMAX * DMAX; e += 256) {
        const int t = e / DMAX, r = e % DMAX;
        hh[e] = (t < d && r < d) ? HHt[t * d + r] : 0.0;
    }
    __syncthreads();
    const int64_t s = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = s < m;
    double w[DMAX], xh[DMAX];
#pragma unroll
    for (int t = 0; t < DMAX; ++t) {
        w[t] = (valid && t < d) ? W[s * d + t] : 0.0;
        xh[t] = (valid && t < d) ? XHt[s * d + t] : 0.0;
    }
    double viol = 0.0;
    if (valid) {
#pragma unroll
        for (int t = 0; t < DMAX; ++t) {
            if (t < d) {
                double g = -xh[t];
#pragma unroll
                for (int r = 0; r < DMAX; ++r)
                    if (r < d) g += hh[t * DMAX + r] * w[r];
                const double pg = w[t] == 0.0 ? (g < 0.0 ? g : 0.0) : g;
                viol += fabs(pg);
                const double hess = hh[t * DMAX + t];
                if (hess != 0.0) {
                    const double v = w[t] - g / hess;
                    w[t] = v > 0.0 ? v : 0.0;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < DMAX; ++t)
            if (t < d) W[s * d + t] = w[t];
    }
    viol = block_sum(viol, red);
    if (threadIdx.x == 0) part[blockIdx.x] = viol;
}

// out[0] = part[0] + part[1] + ... in block order (one thread)
__global__ void nmf_sum_parts(const double* __restrict__ part, int64_t nb, double* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    double s = 0.0;
    for (int64_t b = 0; b < nb; ++b) s += part[b];
    out[0] = s;
}

// ---------------------------------------------------------------------------------------------------------- host driver
// Device state of one NMF problem (the C handle frisk_nmf).  Every buffer is allocated by create.
struct State {
    int device = 0;
    int64_t n = 0, f = 0;
    int d = 0;
    bool frozen = false;                // HHt and XHt hold the products of the current Ht (transform_prepare)
    frisk_common::DevMem mem;
    double *X = nullptr, *W = nullptr, *Ht = nullptr, *XHt = nullptr, *XtW = nullptr, *G = nullptr;
    double *Qn = nullptr, *Qf = nullptr;        // a product's right factor and result: n x NMF_MAX_P, f x NMF_MAX_P
    double *xpart = nullptr, *vpart = nullptr, *viol = nullptr;
    frisk_common::EventTimer<5> timer;
    double ms[3] = {0.0, 0.0, 0.0};     // of the last call: X Q (or X Ht), XT Q' (or XT W), the whole step

    frisk_common::RowSplits xtq_splits() const { return {n, XTQ_SPLITS, XTQ_MIN_ROWS}; }
    int64_t sweep_blocks(int64_t m) const { return (m + 255) / 256; }

    int create(const double* X_in) {
        const size_t sn = size_t(n), sf = size_t(f), sd = size_t(d);
        X = mem.get<double>(sn * sf);
        W = mem.get<double>(sn * sd);
        Ht = mem.get<double>(sf * sd);
        XHt = mem.get<double>(sn * sd);
        XtW = mem.get<double>(sf * sd);
        G = mem.get<double>(sd * sd);
        Qn = mem.get<double>(sn * NMF_MAX_P);
        Qf = mem.get<double>(sf * NMF_MAX_P);
        xpart = mem.get<double>(size_t(xtq_splits().count) * sf * NMF_MAX_P);
        vpart = mem.get<double>(size_t(sweep_blocks(std::max(n, f))));
        viol = mem.get<double>(2);
        if (!X || !W || !Ht || !XHt || !XtW || !G || !Qn || !Qf || !xpart || !vpart || !viol) return -2;
        if (timer.create()) return -2;
        FRISK_HIP_CHECK(hipMemcpy(X, X_in, sn * sf * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(hipMemset(W, 0, sn * sd * sizeof(double)));
        FRISK_HIP_CHECK(hipMemset(Ht, 0, sf * sd * sizeof(double)));
        return 0;
    }

    // Y (n x p, device) = X Q (Q f x p, device)
    void launch_xq(const double* Q, int p, double* Y) {
        for_width<2, 8, 16, NMF_MAX_P>(p, [&](auto pmax) {
            constexpr int PMAX = decltype(pmax)::value, R = PMAX <= 8 ? 4 : PMAX <= 16 ? 2 : 1;         // rows per wave
            hipLaunchKernelGGL((nmf_xq<PMAX, R>), dim3(unsigned((n + 4 * R - 1) / (4 * R))), dim3(256), 0, 0, X, Q, n, f, p, Y);
        });
    }

    // Z (f x p, device) = XT Q (Q n x p, device)
    void launch_xtq(const double* Q, int p, double* Z) {
        const frisk_common::RowSplits sp = xtq_splits();
        const dim3 grid(unsigned((f + 63) / 64), unsigned(sp.count));
        for_width<2, 8, 16, NMF_MAX_P>(p, [&](auto pmax) {
            hipLaunchKernelGGL((nmf_xtq_part<decltype(pmax)::value>), grid, dim3(64), 0, 0, X, Q, n, f, p, sp.rows_per, xpart);
        });
        const int64_t total = f * p;
        hipLaunchKernelGGL(nmf_xtq_reduce, dim3(unsigned((total + 255) / 256)), dim3(256), 0, 0, xpart, int(sp.count), total, Z);
    }

    // One sweep over the m rows of A (m x d) against the Gram matrix in G and the product P (m x d); its violation to out.
    void launch_sweep(double* A, const double* P, int64_t m, double* out) {
        const unsigned nb = unsigned(sweep_blocks(m));
        for_width<2, 4, 8, NMF_MAX_D>(d, [&](auto dmax) {
            hipLaunchKernelGGL((nmf_sweep<decltype(dmax)::value>), dim3(nb), dim3(256), 0, 0, A, G, P, m, d, vpart);
        });
        hipLaunchKernelGGL(nmf_sum_parts, dim3(1), dim3(64), 0, 0, vpart, int64_t(nb), out);
    }

    // Y_out[n][p] = X Q_in[f][p] (host buffers)
    int xq(const double* Q_in, int p, double* Y_out) {
        FRISK_HIP_CHECK(hipMemcpy(Qf, Q_in, size_t(f) * size_t(p) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(timer.record(0));
        launch_xq(Qf, p, Qn);
        FRISK_HIP_CHECK(timer.record(1));
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipMemcpy(Y_out, Qn, size_t(n) * size_t(p) * sizeof(double), hipMemcpyDeviceToHost));
        return timer.elapsed(0, 1, ms[0]);
    }

    // Z_out[f][p] = XT Q_in[n][p] (host buffers)
    int xtq(const double* Q_in, int p, double* Z_out) {
        FRISK_HIP_CHECK(hipMemcpy(Qn, Q_in, size_t(n) * size_t(p) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(timer.record(0));
        launch_xtq(Qn, p, Qf);
        FRISK_HIP_CHECK(timer.record(1));
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipMemcpy(Z_out, Qf, size_t(f) * size_t(p) * sizeof(double), hipMemcpyDeviceToHost));
        return timer.elapsed(0, 1, ms[1]);
    }

    // HHt (in G) and X Ht of the current Ht; they stay valid until Ht changes.
    int prepare() {
        hipLaunchKernelGGL(nmf_gram, dim3(unsigned(d * d)), dim3(256), 0, 0, Ht, f, d, G);
        launch_xq(Ht, d, XHt);
        FRISK_HIP_CHECK(hipGetLastError());
        frozen = true;
        return 0;
    }

    // One iteration of _fit_coordinate_descent: the W sweep, then with update_H the Ht sweep on XT.  violation = the sum of both.
    int step(int update_H, double* violation) {
        FRISK_HIP_CHECK(timer.record(0));
        if (!frozen) {
            hipLaunchKernelGGL(nmf_gram, dim3(unsigned(d * d)), dim3(256), 0, 0, Ht, f, d, G);
            launch_xq(Ht, d, XHt);
        }
        FRISK_HIP_CHECK(timer.record(1));
        launch_sweep(W, XHt, n, viol);
        frozen = !update_H;             // without update_H, G and XHt stay those of the unchanged Ht
        if (update_H) hipLaunchKernelGGL(nmf_gram, dim3(unsigned(d * d)), dim3(256), 0, 0, W, n, d, G);
        FRISK_HIP_CHECK(timer.record(2));
        if (update_H) launch_xtq(W, d, XtW);
        FRISK_HIP_CHECK(timer.record(3));
        if (update_H) launch_sweep(Ht, XtW, f, viol + 1);
        FRISK_HIP_CHECK(timer.record(4));
        FRISK_HIP_CHECK(hipGetLastError());
        double v[2] = {0.0, 0.0};
        FRISK_HIP_CHECK(hipMemcpy(v, viol, (update_H ? 2 : 1) * sizeof(double), hipMemcpyDeviceToHost));
        double total = 0.0;             // sklearn: violation = 0.; violation += (W sweep); violation += (H sweep)
        total += v[0];
        if (update_H) total += v[1];
        *violation = total;
        if (timer.elapsed(0, 1, ms[0]) || timer.elapsed(2, 3, ms[1])) return -2;
        return timer.elapsed(0, 4, ms[2]);
    }
};

}  // namespace frisk_nmf_impl

