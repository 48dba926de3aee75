// mds_kernels.h - metric MDS as the reference's --runProjection MDS runs it (sklearn.manifold.MDS(metric=True, dissimilarity=
// 'euclidean'): euclidean_distances, then SMACOF, sklearn/manifold/_mds.py _smacof_single), FP64.
//
// Layout (n points, input width f >= 1, output dims d <= 64): one n x n buffer D of dissimilarities, computed once per handle and
// read once per SMACOF step; the configuration X_t in one of two n x d buffers.  Every reduction has a fixed order and no
// floating-point atomic, so every output is bit-identical from run to run:
//   dissimilarities  D_ij = sqrt(sum_k (x_ik - x_jk)^2), k in order, by direct differences (the Gram form cancels for close
//                    pairs): 64 x 64 tiles of the upper triangle, f streamed through LDS in chunks of DIS_KC columns, each thread
//                    a 4 x 4 micro-tile; the tile and its mirror are written from the same sums, so D is exactly symmetric, and
//                    the diagonal is exactly 0;
//   one step         for R rows i per block, one pass over j (thread tid takes j = tid, tid + 256, ... in order):
//                    dist_ij = |x_i - x_j| by direct differences, the raw stress terms (dist_ij - D_ij)^2 and dist_ij^2, and
//                    the Guttman sum sum_j ratio_ij (x_i - x_j), ratio_ij = D_ij / (dist_ij == 0 ? 1e-5 : dist_ij), which is
//                    row i of B X without its cancelling diagonal; X_{t+1} = (1 / n) that sum.  Per-thread sums, block_sum
//                    per entry, per-block stress partials summed in block order by one block.
// One pass on X_t yields stress(X_t) and X_{t+1}; the host driver evaluates sklearn's stop rule in double after each pass.
// Included from frisk_analysis.hip after proj_kernels.h; the C entry points there are thin wrappers of the driver below.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "proj_kernels.h"

namespace frisk_mds_impl {

using frisk_proj::block_sum;
using frisk_proj::load_rows;
using frisk_proj::rows_per_block;

constexpr int MAX_D = 64;           // output dims
constexpr int64_t MAX_N = 50000;    // dense n x n FP64 dissimilarities: 20 GB at the cap
constexpr double ZERO_DIST = 1e-5;  // sklearn: distances[distances == 0] = 1e-5
constexpr int DIS_T = 64;           // dissimilarity tile (rows and columns)
constexpr int DIS_KC = 16;          // input columns per LDS chunk

// ---------------------------------------------------------------------------------------------------------- dissimilarities
// Block (bx, by), bx >= by, 256 threads: the tile of rows r0 = 64 by, columns c0 = 64 bx.  Thread (ty, tx) = (tid / 16, tid % 16)
// owns rows r0 + ty + 16 a and columns c0 + tx + 16 b (a, b < 4).  The sums are written to D[r][c] and D[c][r] through one LDS
// transpose, so both halves come from the same value.
__global__ __launch_bounds__(256) void mds_dissimilarities(const double* __restrict__ X, int64_t n, int64_t f,
                                                           double* __restrict__ D) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double A[DIS_KC][DIS_T + 1], B[DIS_KC][DIS_T + 1];
    __shared__ double T[DIS_T][DIS_T + 1];
    const int64_t r0 = int64_t(blockIdx.y) * DIS_T, c0 = int64_t(blockIdx.x) * DIS_T;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double s[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) s[a][b] = 0.0;
    for (int64_t k0 = 0; k0 < f; k0 += DIS_KC) {
        for (int e = threadIdx.x; e < DIS_T * DIS_KC; e += 256) {
            const int r = e / DIS_KC, k = e % DIS_KC;
            const bool kin = k0 + k < f;
            A[k][r] = (kin && r0 + r < n) ? X[(r0 + r) * f + k0 + k] : 0.0;
            B[k][r] = (kin && c0 + r < n) ? X[(c0 + r) * f + k0 + k] : 0.0;
        }
        __syncthreads();
        const int kc = int(f - k0 < DIS_KC ? f - k0 : DIS_KC);
        for (int k = 0; k < kc; ++k) {
            double xa[4], xb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) xa[a] = A[k][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) xb[b] = B[k][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double t = xa[a] - xb[b];
                    s[a][b] += t * t;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int u = ty + 16 * a, v = tx + 16 * b;
            T[u][v] = (r0 + u == c0 + v) ? 0.0 : sqrt(s[a][b]);
        }
    __syncthreads();
    for (int e = threadIdx.x; e < DIS_T * DIS_T; e += 256) {
        const int u = e / DIS_T, v = e % DIS_T;
        if (r0 + u < n && c0 + v < n) D[(r0 + u) * n + c0 + v] = T[u][v];       // the tile, row by row
        if (c0 + u < n && r0 + v < n) D[(c0 + u) * n + r0 + v] = T[v][u];       // its mirror, row by row
    }
}

// ---------------------------------------------------------------------------------------------------------- one SMACOF step
// From X_t = Y: part[2 b] = sum over the block's rows i and all j of (dist_ij - D_ij)^2, part[2 b + 1] = of dist_ij^2; with
// guttman, Ynext[i] = (1 / n) sum_j ratio_ij (y_i - y_j).
template <int MAXD, int R>
__global__ __launch_bounds__(256) void mds_step(const double* __restrict__ Y, const double* __restrict__ D, int64_t n, int d,
                                                int guttman, double* __restrict__ Ynext, double* __restrict__ part) {
    __shared__ double yi[R][MAXD];
    __shared__ double red[4];
    const int64_t i0 = int64_t(blockIdx.x) * R;
    load_rows<MAXD, R>(Y, n, d, i0, yi);
    double acc[R][MAXD];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < MAXD; ++k) acc[r][k] = 0.0;
    double stress = 0.0, sumsq = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        double yj[MAXD];
#pragma unroll
        for (int k = 0; k < MAXD; ++k) yj[k] = k < d ? Y[j * d + k] : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = i0 + r;
            if (i >= n || i == j) continue;
            double diff[MAXD];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < MAXD; ++k) {
                diff[k] = yi[r][k] - yj[k];
                if (k < d) s += diff[k] * diff[k];
            }
            const double dist = sqrt(s);
            const double Dij = D[i * n + j];
            const double e = dist - Dij;
            stress += e * e;
            sumsq += dist * dist;
            if (guttman) {
                const double ratio = Dij / (dist == 0.0 ? ZERO_DIST : dist);
#pragma unroll
                for (int k = 0; k < MAXD; ++k)
                    if (k < d) acc[r][k] += ratio * diff[k];
            }
        }
    }
    if (guttman) {
        const double inv_n = 1.0 / double(n);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int k = 0; k < MAXD; ++k) {
                if (k < d && i0 + r < n) {          // uniform over the block
                    const double s = block_sum(acc[r][k], red);
                    if (threadIdx.x == 0) Ynext[(i0 + r) * d + k] = inv_n * s;
                }
            }
        }
    }
    stress = block_sum(stress, red);
    sumsq = block_sum(sumsq, red);
    if (threadIdx.x == 0) {
        part[2 * int64_t(blockIdx.x)] = stress;
        part[2 * int64_t(blockIdx.x) + 1] = sumsq;
    }
}

// out[0] = sum of part[2 b], out[1] = sum of part[2 b + 1] over b < nb, each in block order (one block)
__global__ __launch_bounds__(256) void mds_sum_parts(const double* __restrict__ part, int64_t nb, double* __restrict__ out) {
    __shared__ double red[4];
    double s0 = 0.0, s1 = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += 256) {
        s0 += part[2 * b];
        s1 += part[2 * b + 1];
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    if (threadIdx.x == 0) {
        out[0] = s0;
        out[1] = s1;
    }
}

// ---------------------------------------------------------------------------------------------------------- host driver
// Device state of one MDS problem (the C handle frisk_mds).  Every buffer is allocated by create.
struct State {
    int device = 0;
    int64_t n = 0, f = 0;
    int d = 0;
    frisk_proj::DevMem mem;
    double *D = nullptr, *Ya = nullptr, *Yb = nullptr, *part = nullptr, *sums = nullptr;

    int64_t step_blocks() const { return (n + rows_per_block(d) - 1) / rows_per_block(d); }

    // Allocates everything and computes D from X.  Returns 0 or -2.
    int create(const double* X_in) {
        const size_t nd = size_t(n) * size_t(d);
        D = mem.get<double>(size_t(n) * size_t(n));
        Ya = mem.get<double>(nd);
        Yb = mem.get<double>(nd);
        part = mem.get<double>(2 * size_t(step_blocks()));
        sums = mem.get<double>(2);
        double* X = mem.get<double>(size_t(n) * size_t(f));
        if (!D || !Ya || !Yb || !part || !sums || !X) return -2;
        FRISK_HIP_CHECK(hipMemcpy(X, X_in, size_t(n) * size_t(f) * sizeof(double), hipMemcpyHostToDevice));
        const unsigned T = unsigned((n + DIS_T - 1) / DIS_T);
        hipLaunchKernelGGL(mds_dissimilarities, dim3(T, T), dim3(256), 0, 0, X, n, f, D);
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipDeviceSynchronize());
        return 0;
    }

    // One pass from Y: stress and sum of squared distances of Y to the host (sums_out[2]); with guttman, Ynext = the next state.
    int step(const double* Y, double* Ynext, int guttman, double* sums_out) {
        const unsigned nb = unsigned(step_blocks());
        frisk_proj::for_rows_per_block<MAX_D>(d, [&](auto maxd, auto r) {
            hipLaunchKernelGGL((mds_step<decltype(maxd)::value, decltype(r)::value>), dim3(nb), dim3(256), 0, 0, Y, D, n, d, guttman, Ynext, part);
        });
        hipLaunchKernelGGL(mds_sum_parts, dim3(1), dim3(256), 0, 0, part, int64_t(nb), sums);
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipMemcpy(sums_out, sums, 2 * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }

    // _smacof_single(D, init=Y0, max_iter, eps) with metric=True.  Returns 0 or -2.
    int run(const double* Y0, int max_iter, double eps, double* Y_out, double* stress_out, int32_t* n_iter_out, double* trace) {
        const size_t bytes = size_t(n) * size_t(d) * sizeof(double);
        FRISK_HIP_CHECK(hipMemcpy(Ya, Y0, bytes, hipMemcpyHostToDevice));
        double* cur = Ya;
        double* nxt = Yb;
        double s[2];
        if (step(cur, nxt, 1, s)) return -2;            // X_1 (the stress of the start is not used)
        std::swap(cur, nxt);
        double old_stress = 0.0, stress = 0.0;
        int it = 0;
        for (;; ++it) {                                  // cur = X_{it + 1}
            const bool last = it + 1 >= max_iter;
            if (step(cur, nxt, last ? 0 : 1, s)) return -2;
            stress = 0.5 * s[0];                         // sklearn: ((distances - disparities) ** 2).sum() / 2
            if (trace) trace[it] = stress;
            if (it > 0 && (old_stress - stress) / (s[1] / 2) < eps) break;
            old_stress = stress;
            if (last) break;
            std::swap(cur, nxt);
        }
        FRISK_HIP_CHECK(hipMemcpy(Y_out, cur, bytes, hipMemcpyDeviceToHost));
        if (stress_out) *stress_out = stress;
        if (n_iter_out) *n_iter_out = it + 1;
        return 0;
    }
};

}  // namespace frisk_mds_impl

