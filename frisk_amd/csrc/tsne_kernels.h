// tsne_kernels.h - exact t-SNE as the reference's PY-TSNE runs it (frisk/tsne.py: x2p L27-80, the loop L126-158), FP64.
//
// Layout (n points, input width f <= 64, output dims d <= 64): one n x n buffer first holds the conditional p_j|i, then the
// symmetric normalised q_ij = max(p_ij, fl(1e-12) / 4).  The reference's P is 4 q while t <= 100 and
// q afterwards, bit for bit (x 4 and / 4 are exact), so q is stored once and multiplied by 4 in the early-exaggeration phase.
// Every reduction has a fixed order and no floating-point atomic, so every output is bit-identical from run to run:
//   affinities  one 1024-thread block per row: distances by direct differences, held in registers, then the reference's
//               bisection on beta, each Hbeta sum a per-thread sum followed by a xor butterfly in each wave and the waves in order;
//               symmetrised tile by tile (32 x 32 tile pairs through LDS), row sums, the rows' total summed by one block;
//   iteration   pass A: sum of num_ij = 1 / (1 + |y_i - y_j|^2) as per-block partials summed in block order by one block;
//               pass B: dY_i = sum_j (P_ij - Q_ij) num_ij (y_i - y_j) for R rows per block (each thread keeps its points in
//               registers and its rows' sums in order, block_sum per entry), and on cost iterations sum P log(P / Q);
//               update: gains, iY, Y per entry, per-block column sums; centring: every block sums the partials in order.
// Included from frisk_analysis.hip; the C entry points there are thin wrappers of the driver below.  block_sum, load_rows and the
// dispatches are analysis_common.h's, shared with MDS.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "analysis_common.h"

namespace frisk_tsne_impl {

using frisk_common::block_sum;
using frisk_common::load_rows;
using frisk_common::rows_per_block;

constexpr int MAX_F = 64;           // input width (the reference's PCA keeps 50 columns)
constexpr int MAX_D = 64;           // output dims
constexpr int64_t MAX_N = 50000;    // dense n x n FP64 buffer: 20 GB at the cap
constexpr int MAX_ITER = 1000;      // tsne.py max_iter
constexpr int MAX_TRIES = 50;       // x2p's bisection cap
constexpr int STOP_EXAGGERATION = 100;      // P /= 4 after this iteration
constexpr int MOMENTUM_SWITCH = 20;         // momentum 0.5 below this iteration, 0.8 from it
constexpr double H_TOL = 1e-5;
constexpr double Q_MIN = 1e-12;             // the clamp of P (x 4 phase) and of Q
constexpr double q_floor() { return Q_MIN * 0.25; }     // fl(1e-12) / 4, exact
constexpr int SYM_T = 32;           // symmetrisation tile
constexpr int ROW_REGS = int((MAX_N + 1023) / 1024);    // distances per thread of the affinity kernel at the largest n

// ---------------------------------------------------------------------------------------------------------- affinities
// One 1024-thread block per row i (its sums: block_sum<16>, the 16 waves in order): D_ij = sum_k (x_ik - x_jk)^2 for j = tid + 1024 c (c < C) kept in registers, the bisection of
// x2p on beta_i (Hbeta without a max-shift: P = exp(-D beta), H = log(sum P) + beta sum(D P) / sum P over j != i), then row i of P
// = p_j|i (0 on the diagonal).  The row is read from X once, whatever the number of tries.  bad is set when the final sum P is
// not a positive finite number (the reference's row would be NaN).
template <int C>
__global__ __launch_bounds__(1024) void tsne_rows(const double* __restrict__ X, int64_t n, int f, double logU, double* __restrict__ P,
                                                  double* __restrict__ beta_out, int32_t* __restrict__ tries_out,
                                                  int32_t* __restrict__ bad) {
    __shared__ double xi[MAX_F];
    __shared__ double red[16];
    const int64_t i = blockIdx.x;
    if (threadIdx.x < f) xi[threadIdx.x] = X[i * f + threadIdx.x];
    __syncthreads();
    double D[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t j = threadIdx.x + int64_t(c) * 1024;
        double s = 0.0;
        if (j < n)
            for (int k = 0; k < f; ++k) {
                const double t = xi[k] - X[j * f + k];
                s += t * t;
            }
        D[c] = s;
    }
    double H = 0.0, sumP = 0.0;
    auto hbeta = [&](double b) {
        double sp = 0.0, sdp = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int64_t j = threadIdx.x + int64_t(c) * 1024;
            if (j < n && j != i) {
                const double p = exp(-D[c] * b);
                sp += p;
                sdp += D[c] * p;
            }
        }
        sumP = block_sum<16>(sp, red);
        sdp = block_sum<16>(sdp, red);
        H = log(sumP) + b * sdp / sumP;
    };
    double beta = 1.0, betamin = -INFINITY, betamax = INFINITY;
    hbeta(beta);
    double Hdiff = H - logU;
    int tries = 0;
    while (fabs(Hdiff) > H_TOL && tries < MAX_TRIES) {      // (a NaN Hdiff stops the loop, as in the reference)
        if (Hdiff > 0.0) {
            betamin = beta;
            beta = (betamax == INFINITY || betamax == -INFINITY) ? beta * 2.0 : (beta + betamax) / 2.0;
        } else {
            betamax = beta;
            beta = (betamin == INFINITY || betamin == -INFINITY) ? beta / 2.0 : (beta + betamin) / 2.0;
        }
        hbeta(beta);
        Hdiff = H - logU;
        ++tries;
    }
    double* row = P + i * n;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t j = threadIdx.x + int64_t(c) * 1024;
        if (j < n) row[j] = j == i ? 0.0 : exp(-D[c] * beta) / sumP;
    }
    if (threadIdx.x == 0) {
        beta_out[i] = beta;
        tries_out[i] = tries;
        if (!(sumP > 0.0) || !isfinite(sumP)) atomicOr(bad, 1);
    }
}

// P + PT in place: block (bx, by), bx >= by, takes the tile pair (by, bx) / (bx, by) through LDS; both get the same sums.
__global__ __launch_bounds__(256) void tsne_symmetrise(double* __restrict__ P, int64_t n) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double a[SYM_T][SYM_T + 1], b[SYM_T][SYM_T + 1];
    const int64_t r0 = int64_t(blockIdx.y) * SYM_T, c0 = int64_t(blockIdx.x) * SYM_T;
    for (int e = threadIdx.x; e < SYM_T * SYM_T; e += 256) {
        const int u = e / SYM_T, v = e % SYM_T;
        if (r0 + u < n && c0 + v < n) a[u][v] = P[(r0 + u) * n + c0 + v];     // a[u][v] = P[r0 + u][c0 + v]
        if (c0 + u < n && r0 + v < n) b[u][v] = P[(c0 + u) * n + r0 + v];     // b[u][v] = P[c0 + u][r0 + v]
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SYM_T * SYM_T; e += 256) {
        const int u = e / SYM_T, v = e % SYM_T;
        if (r0 + u < n && c0 + v < n) P[(r0 + u) * n + c0 + v] = a[u][v] + b[v][u];
        if (c0 + u < n && r0 + v < n) P[(c0 + u) * n + r0 + v] = b[u][v] + a[v][u];
    }
}

// rowsum[i] = sum of row i of P (one block per row)
__global__ __launch_bounds__(256) void tsne_rowsum(const double* __restrict__ P, int64_t n, double* __restrict__ rowsum) {
    __shared__ double red[4];
    const double* row = P + int64_t(blockIdx.x) * n;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) s += row[j];
    s = block_sum(s, red);
    if (threadIdx.x == 0) rowsum[blockIdx.x] = s;
}

// out[0] = sum of v[0 .. m) in a fixed order (one block)
__global__ __launch_bounds__(256) void tsne_sum(const double* __restrict__ v, int64_t m, double* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < m; e += 256) s += v[e];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// q = max(P / total, fl(1e-12) / 4)
__global__ __launch_bounds__(256) void tsne_normalise(double* __restrict__ P, int64_t count, const double* __restrict__ total) {
    const double s = total[0];
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < count; e += int64_t(gridDim.x) * 256)
        P[e] = fmax(P[e] / s, q_floor());
}

// ---------------------------------------------------------------------------------------------------------- one iteration
template <int MAXD>
__device__ inline double num_of(const double* yi, const double* yj, int d) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        if (k < d) {
            const double t = yi[k] - yj[k];
            s += t * t;
        }
    }
    return 1.0 / (1.0 + s);
}

// Pass A: part[b] = sum of num_ij over the block's rows i and all j != i
template <int MAXD, int R>
__global__ __launch_bounds__(256) void tsne_pass_a(const double* __restrict__ Y, int64_t n, int d, double* __restrict__ part) {
    __shared__ double yi[R][MAXD];
    __shared__ double red[4];
    const int64_t i0 = int64_t(blockIdx.x) * R;
    load_rows<MAXD, R>(Y, n, d, i0, yi);
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        double yj[MAXD];
#pragma unroll
        for (int k = 0; k < MAXD; ++k) yj[k] = k < d ? Y[j * d + k] : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (i0 + r < n && i0 + r != j) acc += num_of<MAXD>(yi[r], yj, d);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// Pass B: dY_i = sum_j (P_ij - Q_ij) num_ij (y_i - y_j), P = 4 q (exaggerate) or q, Q = max(num / S, 1e-12);
// with cost: cpart[b] = sum over the block's rows and all j (diagonal included) of P log(P / Q).
template <int MAXD, int R>
__global__ __launch_bounds__(256) void tsne_pass_b(const double* __restrict__ Y, const double* __restrict__ q, int64_t n, int d,
                                                   const double* __restrict__ S, int exaggerate, int cost,
                                                   double* __restrict__ dY, double* __restrict__ cpart) {
    __shared__ double yi[R][MAXD];
    __shared__ double red[4];
    const int64_t i0 = int64_t(blockIdx.x) * R;
    load_rows<MAXD, R>(Y, n, d, i0, yi);
    const double sum = S[0];
    double acc[R][MAXD];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < MAXD; ++k) acc[r][k] = 0.0;
    double c = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        double yj[MAXD];
#pragma unroll
        for (int k = 0; k < MAXD; ++k) yj[k] = k < d ? Y[j * d + k] : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = i0 + r;
            if (i >= n) continue;
            const double qv = q[i * n + j];
            const double p = exaggerate ? qv * 4.0 : qv;
            const double num = i == j ? 0.0 : num_of<MAXD>(yi[r], yj, d);
            const double Q = fmax(num / sum, Q_MIN);
            if (cost) c += p * log(p / Q);
            if (i == j) continue;
            const double coef = (p - Q) * num;
#pragma unroll
            for (int k = 0; k < MAXD; ++k)
                if (k < d) acc[r][k] += coef * (yi[r][k] - yj[k]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < MAXD; ++k) {
            if (k < d && i0 + r < n) {          // uniform over the block
                const double s = block_sum(acc[r][k], red);
                if (threadIdx.x == 0) dY[(i0 + r) * d + k] = s;
            }
        }
    }
    if (cost) {
        c = block_sum(c, red);
        if (threadIdx.x == 0) cpart[blockIdx.x] = c;
    }
}

// gains, iY and Y (not yet centred) of the rows of the block, one thread per row; colpart[b][k] = the block's sum of column k
__global__ __launch_bounds__(256) void tsne_update(double* __restrict__ Y, double* __restrict__ iY, double* __restrict__ gains,
                                                   const double* __restrict__ dY, int64_t n, int d, double momentum,
                                                   double* __restrict__ colpart) {
    __shared__ double red[4];
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    for (int k = 0; k < d; ++k) {
        double y = 0.0;
        if (i < n) {
            const int64_t e = i * d + k;
            const double dy = dY[e], iy = iY[e];
            double g = gains[e];
            g = ((dy > 0.0) != (iy > 0.0)) ? g + 0.2 : g * 0.8;
            if (g < 0.01) g = 0.01;
            const double niy = momentum * iy - 500.0 * (g * dy);
            y = Y[e] + niy;
            gains[e] = g;
            iY[e] = niy;
            Y[e] = y;
        }
        const double s = block_sum(y, red);
        if (threadIdx.x == 0) colpart[int64_t(blockIdx.x) * d + k] = s;
    }
}

// Y -= column means; every block sums the nb column partials in block order (one thread per column)
__global__ __launch_bounds__(256) void tsne_centre(double* __restrict__ Y, int64_t n, int d, const double* __restrict__ colpart,
                                                   int64_t nb) {
    __shared__ double mean[MAX_D];
    if (threadIdx.x < d) {
        double s = 0.0;
        for (int64_t b = 0; b < nb; ++b) s += colpart[b * d + threadIdx.x];
        mean[threadIdx.x] = s / double(n);
    }
    __syncthreads();
    const int64_t count = n * d;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < count; e += int64_t(gridDim.x) * 256) Y[e] -= mean[e % d];
}

// ---------------------------------------------------------------------------------------------------------- host driver
template <int MAXD, int R>
inline void launch_passes(const double* Y, const double* q, int64_t n, int d, double* part, double* S, int exaggerate, int cost,
                          double* dY, double* cpart) {
    const unsigned nb = unsigned((n + R - 1) / R);
    hipLaunchKernelGGL((tsne_pass_a<MAXD, R>), dim3(nb), dim3(256), 0, 0, Y, n, d, part);
    hipLaunchKernelGGL(tsne_sum, dim3(1), dim3(256), 0, 0, part, int64_t(nb), S);
    hipLaunchKernelGGL((tsne_pass_b<MAXD, R>), dim3(nb), dim3(256), 0, 0, Y, q, n, d, S, exaggerate, cost, dY, cpart);
}

// Device state of one t-SNE run (the C handle frisk_tsne).  Every buffer is allocated by create.
struct State {
    int device = 0;
    int64_t n = 0;
    int f = 0, d = 0;
    double perplexity = 0.0;
    bool have_p = false;
    frisk_common::DevMem mem;
    double *X = nullptr, *P = nullptr, *Y = nullptr, *iY = nullptr, *gains = nullptr, *dY = nullptr;
    double *part = nullptr, *S = nullptr, *cpart = nullptr, *colpart = nullptr, *cost = nullptr, *beta = nullptr;
    int32_t *tries = nullptr, *bad = nullptr;

    int64_t pass_blocks() const { return (n + rows_per_block(d) - 1) / rows_per_block(d); }
    int64_t row_blocks() const { return (n + 255) / 256; }

    // Returns 0 or -2.
    int alloc(const double* X_in, const double* Y0) {
        const size_t nd = size_t(n) * size_t(d);
        X = mem.get<double>(size_t(n) * size_t(f));
        P = mem.get<double>(size_t(n) * size_t(n));
        Y = mem.get<double>(nd);
        iY = mem.get<double>(nd);
        gains = mem.get<double>(nd);
        dY = mem.get<double>(nd);
        part = mem.get<double>(size_t(pass_blocks()));
        S = mem.get<double>(1);
        cpart = mem.get<double>(size_t(pass_blocks()));
        colpart = mem.get<double>(size_t(row_blocks()) * size_t(d));
        cost = mem.get<double>(MAX_ITER / 10);
        beta = mem.get<double>(size_t(n));
        tries = mem.get<int32_t>(size_t(n));
        bad = mem.get<int32_t>(1);
        if (!X || !P || !Y || !iY || !gains || !dY || !part || !S || !cpart || !colpart || !cost || !beta || !tries || !bad) return -2;
        FRISK_HIP_CHECK(hipMemcpy(X, X_in, size_t(n) * size_t(f) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(hipMemcpy(Y, Y0, nd * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(hipMemset(iY, 0, nd * sizeof(double)));
        std::vector<double> ones(nd, 1.0);
        FRISK_HIP_CHECK(hipMemcpy(gains, ones.data(), nd * sizeof(double), hipMemcpyHostToDevice));
        return 0;
    }

    // P = q.  Returns 0, -1 (a row's sum P is 0 or not finite) or -2.
    int affinities() {
        FRISK_HIP_CHECK(hipMemset(bad, 0, sizeof(int32_t)));
        const double logU = std::log(perplexity);
        frisk_common::for_width<1, 8, ROW_REGS>(int((n + 1023) / 1024), [&](auto c) {
            hipLaunchKernelGGL(tsne_rows<decltype(c)::value>, dim3(unsigned(n)), dim3(1024), 0, 0, X, n, f, logU, P, beta, tries, bad);
        });
        const unsigned T = unsigned((n + SYM_T - 1) / SYM_T);
        hipLaunchKernelGGL(tsne_symmetrise, dim3(T, T), dim3(256), 0, 0, P, n);
        double* rowsum = dY;            // n entries are free here only if d >= 1: dY holds n * d >= n
        hipLaunchKernelGGL(tsne_rowsum, dim3(unsigned(n)), dim3(256), 0, 0, P, n, rowsum);
        hipLaunchKernelGGL(tsne_sum, dim3(1), dim3(256), 0, 0, rowsum, n, S);
        const int64_t count = n * n;
        hipLaunchKernelGGL(tsne_normalise, dim3(unsigned(std::min<int64_t>((count + 255) / 256, 65536))), dim3(256), 0, 0, P, count, S);
        FRISK_HIP_CHECK(hipGetLastError());
        int32_t flag = 0;
        FRISK_HIP_CHECK(hipMemcpy(&flag, bad, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (flag) return -1;
        have_p = true;
        return 0;
    }

    // Iterations t = t0 .. t1 - 1 on one stream, no host sync inside; cost_out gets one value per t with (t + 1) % 10 == 0.
    int run(int t0, int t1, double* cost_out) {
        const int64_t nrb = row_blocks();
        for (int t = t0; t < t1; ++t) {
            const int exaggerate = t <= STOP_EXAGGERATION;
            const int with_cost = (t + 1) % 10 == 0;
            frisk_common::for_rows_per_block<MAX_D>(d, [&](auto maxd, auto r) {
                launch_passes<decltype(maxd)::value, decltype(r)::value>(Y, P, n, d, part, S, exaggerate, with_cost, dY, cpart);
            });
            if (with_cost) hipLaunchKernelGGL(tsne_sum, dim3(1), dim3(256), 0, 0, cpart, pass_blocks(), cost + (t + 1) / 10 - 1);
            hipLaunchKernelGGL(tsne_update, dim3(unsigned(nrb)), dim3(256), 0, 0, Y, iY, gains, dY, n, d,
                               t < MOMENTUM_SWITCH ? 0.5 : 0.8, colpart);
            hipLaunchKernelGGL(tsne_centre, dim3(unsigned(std::min<int64_t>((n * d + 255) / 256, 1024))), dim3(256), 0, 0, Y, n, d,
                               colpart, nrb);
        }
        FRISK_HIP_CHECK(hipGetLastError());
        const int c0 = t0 / 10, c1 = t1 / 10;        // cost slots (t + 1) / 10 - 1 of t0 <= t < t1
        if (cost_out && c1 > c0)
            FRISK_HIP_CHECK(hipMemcpy(cost_out, cost + c0, size_t(c1 - c0) * sizeof(double), hipMemcpyDeviceToHost));
        FRISK_HIP_CHECK(hipDeviceSynchronize());
        return 0;
    }
};

}  // namespace frisk_tsne_impl

