// skltsne_kernels.h - sklearn 1.7's TSNE as the reference runs it under --runProjection SKL-TSNE (frisk/__init__.py L1606-1621):
// method='exact' and method='barnes_hut', the latter with the repulsive term summed over all pairs (sklearn's own angle -> 0 limit,
// not its angle = 0.5 tree walk: DESIGN.md section 9.6).  The embedding Y, the update and the gains are float32, as sklearn holds
// them, and the update arithmetic is float32 in sklearn's order of operations; the gradient, the normaliser and the error are
// accumulated in FP64 and the gradient is rounded to float32 once before the gains rule.  A double copy of Y (exactly the float32
// values) is kept beside it, so the passes read their rows through analysis_common.h's load_rows.
//
// Every reduction has a fixed order and no floating-point atomic, so every output is bit-identical from run to run:
//   dense affinities   squared distances by direct differences, rounded to float32 (pair_tile, any width f), then one 1024-thread
//                      block per row: the row in registers as float32, sklearn's _binary_search_perplexity as written (beta from 1,
//                      at most 100 steps, tolerance (float)1e-5, an all-zero row sum replaced by (float)1e-8), the row of p_j|i;
//                      P + PT tile by tile, its total, P = max(P / max(total, eps64), eps64) off the diagonal;
//   sparse affinities  one 1024-thread block per row: the row's float32 distances in registers, the k-th smallest of the keys
//                      (distance bits, column) found bit by bit with block-wide counts (ties go to the lower column), the k kept
//                      columns written in column order by a block-wide scan, the same bisection over the kept distances only;
//                      the caller symmetrises the n x k conditionals on the host and uploads the CSR (float32 values);
//   iteration          all pairs: the sum of the Student kernel per block, the blocks summed in order by one block (the sparse form
//                      also keeps sum_j kernel^2 (y_i - y_j) per row in the same pass); dense P: the gradient rows and the KL sum;
//                      CSR P: one wave per row over its neighbours; the float32 update with gains, per-block sums of squares of
//                      grad * gains for the norm.
// Included from frisk_analysis.hip; the C entry points there are thin wrappers of the State below.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "analysis_common.h"

namespace frisk_skltsne_impl {

using frisk_common::block_sum;
using frisk_common::load_rows;
using frisk_common::rows_per_block;
using frisk_common::wave_sum;

constexpr int MAX_D = 64;           // output dims of the exact method
constexpr int MAX_D_BH = 3;         // sklearn: n_components < 4 for barnes_hut
constexpr int64_t MAX_N = 50000;    // dense n x n FP64 buffer: 20 GB at the cap
constexpr int MAX_ITER = 1000;
constexpr int N_STEPS = 100;        // _binary_search_perplexity's cap
constexpr int SYM_T = 32;           // symmetrisation tile
constexpr int ROW_REGS = int((MAX_N + 1023) / 1024);    // distances per thread of a row kernel at the largest n
constexpr int METHOD_EXACT = 0, METHOD_BARNES_HUT = 1;
constexpr double EPS64 = DBL_EPSILON;                   // MACHINE_EPSILON / FLOAT64_EPS
constexpr double TINY32 = double(FLT_MIN);              // FLOAT32_TINY

// pair_tile's value of a pair: sklearn casts the squared distances to float32 before the search
struct RoundedToF32 {
    __device__ double operator()(double s) const { return double(float(s)); }
};

// ---------------------------------------------------------------------------------------------------------- affinities
// block-wide sum of an int over 16 waves, in a fixed order
__device__ inline int block_count(int v, int* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += red[w];
    __syncthreads();
    return s;
}

// _binary_search_perplexity for one row held by a 1024-thread block: D[c] is the float32 squared distance of the thread's c-th
// element and act(c) says whether it takes part.  On return every thread holds beta (the one the final probabilities belong to:
// sklearn moves beta once more after the 100th evaluation and keeps the probabilities of the one before), sumP and the number of
// the step that met the tolerance (100: none did).  The probability of an element is exp(-D beta) / sumP.
template <int C, typename Active>
__device__ inline void bisect(const float (&D)[C], Active act, double logU, double* red, double& beta_used, double& sumP, int& steps) {
    const double tol = double(1e-5f);           // cdef float PERPLEXITY_TOLERANCE
    double beta = 1.0, bmin = -INFINITY, bmax = INFINITY;
    int l = 0;
    beta_used = beta;
    sumP = 0.0;
    for (; l < N_STEPS; ++l) {
        double sp = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (act(c)) sp += exp(-double(D[c]) * beta);
        sumP = block_sum<16>(sp, red);
        if (sumP == 0.0) sumP = double(1e-8f);  // cdef float EPSILON_DBL
        double sdp = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (act(c)) sdp += double(D[c]) * (exp(-double(D[c]) * beta) / sumP);
        sdp = block_sum<16>(sdp, red);
        const double diff = log(sumP) + beta * sdp - logU;
        beta_used = beta;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == INFINITY ? beta * 2.0 : (beta + bmax) / 2.0;
        } else {
            bmax = beta;
            beta = bmin == -INFINITY ? beta / 2.0 : (beta + bmin) / 2.0;
        }
    }
    steps = l;
}

// Dense form.  Row i of P holds the float32-rounded squared distances on entry and p_j|i on return (0 on the diagonal).
template <int C>
__global__ __launch_bounds__(1024) void skl_rows_dense(double* __restrict__ P, int64_t n, double logU, double* __restrict__ beta_out,
                                                       int32_t* __restrict__ steps_out) {
    __shared__ double red[16];
    const int64_t i = blockIdx.x;
    double* row = P + i * n;
    float D[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t j = threadIdx.x + int64_t(c) * 1024;
        D[c] = j < n ? float(row[j]) : 0.f;
    }
    auto act = [&](int c) {
        const int64_t j = threadIdx.x + int64_t(c) * 1024;
        return j < n && j != i;
    };
    double beta, sumP;
    int steps;
    bisect<C>(D, act, logU, red, beta, sumP, steps);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t j = threadIdx.x + int64_t(c) * 1024;
        if (j < n) row[j] = j == i ? 0.0 : exp(-double(D[c]) * beta) / sumP;
    }
    if (threadIdx.x == 0) {
        beta_out[i] = beta;
        steps_out[i] = steps;
    }
}

// Sparse form.  Row i: the float32 squared distances to every other row by direct differences (k in order), the k nearest (ties to
// the lower column) in column order into idx[i][0 .. k), and their p_j|i from the bisection over those k only into cond[i][0 .. k).
template <int C>
__global__ __launch_bounds__(1024) void skl_rows_knn(const double* __restrict__ X, int64_t n, int64_t f, int k, double logU,
                                                     int32_t* __restrict__ idx, double* __restrict__ cond,
                                                     double* __restrict__ beta_out, int32_t* __restrict__ steps_out) {
    __shared__ double red[16];
    __shared__ int cnt[16];
    const int64_t i = blockIdx.x;
    const double* xi = X + i * f;
    float D[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t j = threadIdx.x + int64_t(c) * 1024;
        double s = 0.0;
        if (j < n && j != i) {
            const double* xj = X + j * f;
            for (int64_t q = 0; q < f; ++q) {
                const double t = xi[q] - xj[q];
                s += t * t;
            }
        }
        D[c] = float(s);
    }
    // a non-negative float orders as its bits; the column breaks ties and makes every key distinct (j < 65 536)
    auto key = [&](int c) {
        const int64_t j = threadIdx.x + int64_t(c) * 1024;
        return (j < n && j != i) ? ((unsigned long long)(__float_as_uint(D[c])) << 32) | (unsigned long long)(j) : ~0ull;
    };
    // T = the k-th smallest key: the largest T with fewer than k keys below it, built from the top bit down.  Bit 63 (the sign) and
    // bits 16 .. 31 (columns are below 65 536) are 0 in every key of a row.
    unsigned long long T = 0;
    for (int bit = 62; bit >= 0; --bit) {
        if (bit == 31) bit = 15;
        const unsigned long long trial = T | (1ull << bit);
        int below = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) below += key(c) < trial ? 1 : 0;
        if (block_count(below, cnt) < k) T = trial;
    }
    auto act = [&](int c) { return key(c) <= T; };
    double beta, sumP;
    int steps;
    bisect<C>(D, act, logU, red, beta, sumP, steps);
    // the kept columns in column order: element (c, tid) is column tid + 1024 c, so chunk by chunk, and a scan inside each chunk
    int base = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const bool keep = act(c);
        const unsigned long long b = __ballot(keep);
        const int within = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) cnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += cnt[w];
            total += cnt[w];
        }
        __syncthreads();
        const int pos = base + before + within;
        if (keep && pos < k) {
            idx[i * k + pos] = int32_t(threadIdx.x + c * 1024);
            cond[i * k + pos] = exp(-double(D[c]) * beta) / sumP;
        }
        base += total;
    }
    if (threadIdx.x == 0) {
        beta_out[i] = beta;
        steps_out[i] = steps;
    }
}

// P + PT in place: block (bx, by), bx >= by, takes the tile pair (by, bx) / (bx, by) through LDS; both get the same sums.
__global__ __launch_bounds__(256) void skl_symmetrise(double* __restrict__ P, int64_t n) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double a[SYM_T][SYM_T + 1], b[SYM_T][SYM_T + 1];
    const int64_t r0 = int64_t(blockIdx.y) * SYM_T, c0 = int64_t(blockIdx.x) * SYM_T;
    for (int e = threadIdx.x; e < SYM_T * SYM_T; e += 256) {
        const int u = e / SYM_T, v = e % SYM_T;
        a[u][v] = (r0 + u < n && c0 + v < n) ? P[(r0 + u) * n + c0 + v] : 0.0;
        b[u][v] = (c0 + u < n && r0 + v < n) ? P[(c0 + u) * n + r0 + v] : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SYM_T * SYM_T; e += 256) {
        const int u = e / SYM_T, v = e % SYM_T;
        if (r0 + u < n && c0 + v < n) P[(r0 + u) * n + c0 + v] = a[u][v] + b[v][u];
        if (c0 + u < n && r0 + v < n) P[(c0 + u) * n + r0 + v] = b[u][v] + a[v][u];
    }
}

// rowsum[i] = sum of row i of P (one block per row)
__global__ __launch_bounds__(256) void skl_rowsum(const double* __restrict__ P, int64_t n, double* __restrict__ rowsum) {
    __shared__ double red[4];
    const double* row = P + int64_t(blockIdx.x) * n;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) s += row[j];
    s = block_sum(s, red);
    if (threadIdx.x == 0) rowsum[blockIdx.x] = s;
}

// out[0] = sum of v[0 .. m) in a fixed order (one block)
__global__ __launch_bounds__(256) void skl_sum(const double* __restrict__ v, int64_t m, double* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < m; e += 256) s += v[e];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// P = max(P / max(total, eps64), eps64) off the diagonal (sklearn's condensed form has no diagonal: it stays 0 here)
__global__ __launch_bounds__(256) void skl_normalise(double* __restrict__ P, int64_t n, const double* __restrict__ total) {
    const double s = fmax(total[0], EPS64);
    const int64_t count = n * n;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < count; e += int64_t(gridDim.x) * 256)
        P[e] = (e / n == e % n) ? 0.0 : fmax(P[e] / s, EPS64);
}

// ---------------------------------------------------------------------------------------------------------- one iteration
// The Student kernel of a pair from s = |y_i - y_j|^2 (FP64).  exact: (1 + s / dof) ^ (-(dof + 1) / 2) (_kl_divergence);
// barnes_hut: (dof / (dof + s)) ^ ((dof + 1) / 2) (_barnes_hut_tsne.pyx); neither raises to a power when dof is 1.
template <bool BH>
__device__ inline double student(double s, int dof) {
    const double fd = double(dof);
    if (BH) {
        const double q = fd / (fd + s);
        return dof == 1 ? q : pow(q, (fd + 1.0) / 2.0);
    }
    const double t = s / fd + 1.0;
    return dof == 1 ? 1.0 / t : pow(t, (fd + 1.0) / -2.0);
}

// s = |y_i - y_j|^2 and diff[k] = y_i[k] - y_j[k] rounded to float32, which is what sklearn multiplies the weights with (exact:
// X_embedded[i] - X_embedded is a float32 array; barnes_hut: buff is float)
template <int MAXD>
__device__ inline double sq_diff(const double* yi, const double* yj, int d, double* diff) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        if (k < d) {
            const double t = yi[k] - yj[k];
            s += t * t;
            diff[k] = double(float(t));
        }
    }
    return s;
}

// All pairs: part[b] = sum of the kernel over the block's rows i and all j != i.  BH: also neg[i][k] = sum_j kernel^2 diff_k
// (compute_gradient_negative with every leaf visited: mult = qijZ * qijZ after the power).
template <int MAXD, int R, bool BH>
__global__ __launch_bounds__(256) void skl_pass_a(const double* __restrict__ Y, int64_t n, int d, int dof, double* __restrict__ part,
                                                  double* __restrict__ neg) {
    __shared__ double yi[R][MAXD];
    __shared__ double red[4];
    const int64_t i0 = int64_t(blockIdx.x) * R;
    load_rows<MAXD, R>(Y, n, d, i0, yi);
    double acc = 0.0;
    double nacc[BH ? R : 1][BH ? MAXD : 1];
    if (BH) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < MAXD; ++k) nacc[BH ? r : 0][BH ? k : 0] = 0.0;
    }
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        double yj[MAXD];
#pragma unroll
        for (int k = 0; k < MAXD; ++k) yj[k] = k < d ? Y[j * d + k] : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (i0 + r >= n || i0 + r == j) continue;
            double diff[MAXD];
            const double q = student<BH>(sq_diff<MAXD>(yi[r], yj, d, diff), dof);
            acc += q;
            if (BH) {
                const double m = q * q;
#pragma unroll
                for (int k = 0; k < MAXD; ++k)
                    if (k < d) nacc[BH ? r : 0][BH ? k : 0] += m * diff[k];
            }
        }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
    if (BH) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int k = 0; k < MAXD; ++k) {
                if (k < d && i0 + r < n) {          // uniform over the block
                    const double s = block_sum(nacc[BH ? r : 0][BH ? k : 0], red);
                    if (threadIdx.x == 0) neg[(i0 + r) * d + k] = s;
                }
            }
        }
    }
}

// Dense P (_kl_divergence): grad_i = fl32(fl32(sum_j (p_ij - Q_ij) num_ij diff_ij) * c), p = ex P, Q = max(num / S, eps64); with
// cost: cpart[b] = sum over the block's rows and all j != i of p log(max(p, eps64) / Q).
template <int MAXD, int R>
__global__ __launch_bounds__(256) void skl_pass_b(const double* __restrict__ Y, const double* __restrict__ P, int64_t n, int d, int dof,
                                                  const double* __restrict__ S, double ex, float c32, int cost,
                                                  float* __restrict__ grad, double* __restrict__ cpart) {
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
    double kl = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        double yj[MAXD];
#pragma unroll
        for (int k = 0; k < MAXD; ++k) yj[k] = k < d ? Y[j * d + k] : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = i0 + r;
            if (i >= n || i == j) continue;
            double diff[MAXD];
            const double num = student<false>(sq_diff<MAXD>(yi[r], yj, d, diff), dof);
            const double p = P[i * n + j] * ex;
            const double Q = fmax(num / sum, EPS64);
            if (cost) kl += p * log(fmax(p, EPS64) / Q);
            const double coef = (p - Q) * num;
#pragma unroll
            for (int k = 0; k < MAXD; ++k)
                if (k < d) acc[r][k] += coef * diff[k];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < MAXD; ++k) {
            if (k < d && i0 + r < n) {          // uniform over the block
                const double s = block_sum(acc[r][k], red);
                if (threadIdx.x == 0) grad[(i0 + r) * d + k] = float(s) * c32;
            }
        }
    }
    if (cost) {
        kl = block_sum(kl, red);
        if (threadIdx.x == 0) cpart[blockIdx.x] = kl;
    }
}

// CSR P (compute_gradient_positive and compute_gradient): one wave per row i over its neighbours, lane l taking entries l, l + 64,
// ...: pos_k = sum p q diff_k, grad_i = fl32(fl32(pos - neg_i / max(S, eps64)) * c), and with cost cpart[i] = sum p log(max(p,
// tiny32) / max(q / max(S, eps64), tiny32)).  p = fl32(val * ex) as sklearn hands the exaggerated values over in float32.
__global__ __launch_bounds__(64) void skl_pos_csr(const double* __restrict__ Y, const int64_t* __restrict__ indptr,
                                                  const int32_t* __restrict__ indices, const float* __restrict__ val, int64_t n, int d,
                                                  int dof, const double* __restrict__ S, const double* __restrict__ neg, float ex32,
                                                  float c32, int cost, float* __restrict__ grad, double* __restrict__ cpart) {
    const int64_t i = blockIdx.x;
    const double sum = fmax(S[0], EPS64);
    double yi[4], pos[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) yi[k] = k < d ? Y[i * d + k] : 0.0;
    double kl = 0.0;
    for (int64_t e = indptr[i] + threadIdx.x; e < indptr[i + 1]; e += 64) {
        const int64_t j = indices[e];
        double yj[4], diff[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) yj[k] = k < d ? Y[j * d + k] : 0.0;
        const double q = student<true>(sq_diff<4>(yi, yj, d, diff), dof);
        const double p = double(val[e] * ex32);
        if (cost) kl += p * log(fmax(p, TINY32) / fmax(q / sum, TINY32));
        const double w = p * q;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < d) pos[k] += w * diff[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < d) {
            const double s = wave_sum(pos[k]);
            if (threadIdx.x == 0) grad[i * d + k] = float(s - neg[i * d + k] / sum) * c32;
        }
    }
    if (cost) {
        kl = wave_sum(kl);
        if (threadIdx.x == 0) cpart[i] = kl;
    }
}

// _gradient_descent's update in float32, in its order: inc = update * grad < 0; gains += 0.2 or *= 0.8; clip below at min_gain;
// grad *= gains; update = momentum * update - learning_rate * grad; Y += update.  Yd gets the new Y as doubles, and npart[b] the
// block's sum of squares of grad * gains (FP64), for the norm.
__global__ __launch_bounds__(256) void skl_update(float* __restrict__ Y, float* __restrict__ U, float* __restrict__ G,
                                                  const float* __restrict__ grad, double* __restrict__ Yd, int64_t count, float momentum,
                                                  float rate, double* __restrict__ npart) {
    __shared__ double red[4];
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    double sq = 0.0;
    if (e < count) {
        const float g = grad[e], u = U[e];
        float gain = G[e];
        gain = (u * g < 0.0f) ? gain + 0.2f : gain * 0.8f;
        if (gain < 0.01f) gain = 0.01f;
        const float gg = g * gain;
        const float mu = momentum * u, rg = rate * gg;
        const float nu = mu - rg;
        const float y = Y[e] + nu;
        G[e] = gain;
        U[e] = nu;
        Y[e] = y;
        Yd[e] = double(y);
        sq = double(gg) * double(gg);
    }
    sq = block_sum(sq, red);
    if (threadIdx.x == 0) npart[blockIdx.x] = sq;
}

// Yd = Y as doubles (after set(), and after the affinities borrowed Yd for their row sums)
__global__ __launch_bounds__(256) void refresh_double(const float* __restrict__ Y, double* __restrict__ Yd, int64_t count) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e < count) Yd[e] = double(Y[e]);
}

// ---------------------------------------------------------------------------------------------------------- host driver
// Device state of one run (the C handle frisk_skltsne).
struct State {
    int device = 0;
    int64_t n = 0, f = 0;
    int d = 0, method = METHOD_EXACT, k = 0;
    double perplexity = 0.0;
    bool have_aff = false, have_p = false;
    double ms[3] = {-1.0, -1.0, -1.0};         // affinities, the last run, unused
    frisk_common::DevMem mem, csr;
    frisk_common::EventTimer<2> timer;
    double *X = nullptr, *P = nullptr, *cond = nullptr, *Yd = nullptr, *neg = nullptr, *part = nullptr, *S = nullptr, *cpart = nullptr;
    double *npart = nullptr, *out2 = nullptr, *beta = nullptr;
    float *Y = nullptr, *U = nullptr, *G = nullptr, *grad = nullptr, *val = nullptr;
    int32_t *idx = nullptr, *steps = nullptr, *indices = nullptr;
    int64_t* indptr = nullptr;

    int dof() const { return std::max(d - 1, 1); }
    int64_t pass_blocks() const { return (n + rows_per_block(d) - 1) / rows_per_block(d); }
    int64_t update_blocks() const { return (n * d + 255) / 256; }

    // Returns 0 or -2.  Y starts at 0, the update at 0 and the gains at 1; the caller sets its start with set().
    int create(const double* X_in) {
        const size_t nd = size_t(n) * size_t(d);
        k = int(std::min<int64_t>(n - 1, int64_t(3.0 * perplexity + 1.0)));
        X = mem.get<double>(size_t(n) * size_t(f));
        if (method == METHOD_EXACT) {
            P = mem.get<double>(size_t(n) * size_t(n));
        } else {
            idx = mem.get<int32_t>(size_t(n) * size_t(k));
            cond = mem.get<double>(size_t(n) * size_t(k));
            neg = mem.get<double>(nd);
        }
        Yd = mem.get<double>(std::max(nd, size_t(n)));          // (its first n entries serve as the row sums of the affinities)
        Y = mem.get<float>(nd);
        U = mem.get<float>(nd);
        G = mem.get<float>(nd);
        grad = mem.get<float>(nd);
        part = mem.get<double>(size_t(pass_blocks()));
        cpart = mem.get<double>(size_t(std::max(pass_blocks(), n)));
        npart = mem.get<double>(size_t(update_blocks()));
        S = mem.get<double>(1);
        out2 = mem.get<double>(2);
        beta = mem.get<double>(size_t(n));
        steps = mem.get<int32_t>(size_t(n));
        if (!X || !(P || (idx && cond && neg)) || !Yd || !Y || !U || !G || !grad || !part || !cpart || !npart || !S || !out2 || !beta ||
            !steps)
            return -2;
        if (timer.create()) return -2;
        FRISK_HIP_CHECK(hipMemcpy(X, X_in, size_t(n) * size_t(f) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(hipMemset(Yd, 0, std::max(nd, size_t(n)) * sizeof(double)));
        FRISK_HIP_CHECK(hipMemset(Y, 0, nd * sizeof(float)));
        FRISK_HIP_CHECK(hipMemset(U, 0, nd * sizeof(float)));
        std::vector<float> ones(nd, 1.0f);
        FRISK_HIP_CHECK(hipMemcpy(G, ones.data(), nd * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }

    // The conditional (sparse) or joint (dense) probabilities, once.  Returns 0 or -2.
    int affinities() {
        if (have_aff) return 0;
        const double logU = std::log(double(float(perplexity)));        // (float desired_perplexity)
        const int chunks = int((n + 1023) / 1024);
        FRISK_HIP_CHECK(timer.record(0));
        if (method == METHOD_EXACT) {
            const unsigned T = unsigned((n + frisk_common::PAIR_T - 1) / frisk_common::PAIR_T);
            hipLaunchKernelGGL((frisk_common::pair_tile<RoundedToF32, int64_t>), dim3(T, T), dim3(256), 0, 0, X, n, f, RoundedToF32(), P);
            frisk_common::for_width<1, 8, ROW_REGS>(chunks, [&](auto c) {
                hipLaunchKernelGGL(skl_rows_dense<decltype(c)::value>, dim3(unsigned(n)), dim3(1024), 0, 0, P, n, logU, beta, steps);
            });
            const unsigned Ts = unsigned((n + SYM_T - 1) / SYM_T);
            hipLaunchKernelGGL(skl_symmetrise, dim3(Ts, Ts), dim3(256), 0, 0, P, n);
            double* rowsum = Yd;
            hipLaunchKernelGGL(skl_rowsum, dim3(unsigned(n)), dim3(256), 0, 0, P, n, rowsum);
            hipLaunchKernelGGL(skl_sum, dim3(1), dim3(256), 0, 0, rowsum, n, S);
            hipLaunchKernelGGL(skl_normalise, dim3(unsigned(std::min<int64_t>((n * n + 255) / 256, 65536))), dim3(256), 0, 0, P, n, S);
            hipLaunchKernelGGL(refresh_double, dim3(unsigned(update_blocks())), dim3(256), 0, 0, Y, Yd, n * d);
            have_p = true;
        } else {
            frisk_common::for_width<1, 8, ROW_REGS>(chunks, [&](auto c) {
                hipLaunchKernelGGL(skl_rows_knn<decltype(c)::value>, dim3(unsigned(n)), dim3(1024), 0, 0, X, n, f, k, logU, idx, cond,
                                   beta, steps);
            });
        }
        FRISK_HIP_CHECK(timer.record(1));
        FRISK_HIP_CHECK(hipGetLastError());
        if (timer.elapsed(0, 1, ms[0])) return -2;
        have_aff = true;
        return 0;
    }

    // The symmetrised joint probabilities of the sparse form (validated by the caller).  Returns 0 or -2.
    int set_p(const int64_t* ip, const int32_t* ind, const float* v, int64_t nnz) {
        frisk_common::DevMem fresh;
        int64_t* a = fresh.get<int64_t>(size_t(n) + 1);
        int32_t* b = fresh.get<int32_t>(size_t(nnz));
        float* c = fresh.get<float>(size_t(nnz));
        if (!a || !b || !c) return -2;
        FRISK_HIP_CHECK(hipMemcpy(a, ip, (size_t(n) + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        if (nnz) {
            FRISK_HIP_CHECK(hipMemcpy(b, ind, size_t(nnz) * sizeof(int32_t), hipMemcpyHostToDevice));
            FRISK_HIP_CHECK(hipMemcpy(c, v, size_t(nnz) * sizeof(float), hipMemcpyHostToDevice));
        }
        FRISK_HIP_CHECK(hipDeviceSynchronize());
        std::swap(csr.ptrs, fresh.ptrs);        // (the previous arrays, if any, are freed with `fresh`)
        indptr = a; indices = b; val = c;
        have_p = true;
        return 0;
    }

    int refresh() {
        hipLaunchKernelGGL(refresh_double, dim3(unsigned(update_blocks())), dim3(256), 0, 0, Y, Yd, n * d);
        FRISK_HIP_CHECK(hipGetLastError());
        return 0;
    }

    // Iterations t0 .. t1 - 1 (t1 > t0) on one stream, no host sync inside; the error and the norm of grad * gains of the last one.
    int run(int t0, int t1, double momentum, double exaggeration, double* error, double* grad_norm) {
        const int dof_ = dof();
        const float c32 = float(2.0 * (dof_ + 1.0) / dof_);
        const unsigned nb = unsigned(pass_blocks()), ub = unsigned(update_blocks());
        FRISK_HIP_CHECK(timer.record(0));
        for (int t = t0; t < t1; ++t) {
            const int cost = t == t1 - 1;
            if (method == METHOD_EXACT) {
                frisk_common::for_rows_per_block<MAX_D>(d, [&](auto maxd, auto r) {
                    constexpr int M = decltype(maxd)::value, R = decltype(r)::value;
                    hipLaunchKernelGGL((skl_pass_a<M, R, false>), dim3(nb), dim3(256), 0, 0, Yd, n, d, dof_, part, (double*)nullptr);
                    hipLaunchKernelGGL(skl_sum, dim3(1), dim3(256), 0, 0, part, int64_t(nb), S);
                    hipLaunchKernelGGL((skl_pass_b<M, R>), dim3(nb), dim3(256), 0, 0, Yd, P, n, d, dof_, S, exaggeration, c32, cost,
                                       grad, cpart);
                });
                if (cost) hipLaunchKernelGGL(skl_sum, dim3(1), dim3(256), 0, 0, cpart, int64_t(nb), out2);
            } else {
                hipLaunchKernelGGL((skl_pass_a<4, rows_per_block(4), true>), dim3(nb), dim3(256), 0, 0, Yd, n, d, dof_, part, neg);
                hipLaunchKernelGGL(skl_sum, dim3(1), dim3(256), 0, 0, part, int64_t(nb), S);
                hipLaunchKernelGGL(skl_pos_csr, dim3(unsigned(n)), dim3(64), 0, 0, Yd, indptr, indices, val, n, d, dof_, S, neg,
                                   float(exaggeration), c32, cost, grad, cpart);
                if (cost) hipLaunchKernelGGL(skl_sum, dim3(1), dim3(256), 0, 0, cpart, n, out2);
            }
            hipLaunchKernelGGL(skl_update, dim3(ub), dim3(256), 0, 0, Y, U, G, grad, Yd, n * d, float(momentum), 1000.0f, npart);
        }
        hipLaunchKernelGGL(skl_sum, dim3(1), dim3(256), 0, 0, npart, int64_t(ub), out2 + 1);
        FRISK_HIP_CHECK(timer.record(1));
        FRISK_HIP_CHECK(hipGetLastError());
        double host[2];
        FRISK_HIP_CHECK(hipMemcpy(host, out2, sizeof(host), hipMemcpyDeviceToHost));
        if (timer.elapsed(0, 1, ms[1])) return -2;
        *error = host[0];
        *grad_norm = std::sqrt(host[1]);
        return 0;
    }
};

}  // namespace frisk_skltsne_impl
