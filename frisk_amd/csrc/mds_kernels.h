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
// Included from frisk_analysis.hip; the C entry points there are thin wrappers of the driver below.  The tile kernel of the
// dissimilarities is analysis_common.h's pair_tile, shared with the spectral affinities; block_sum and load_rows are shared with t-SNE.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "analysis_common.h"

namespace frisk_mds_impl {

using frisk_common::block_sum;
using frisk_common::load_rows;
using frisk_common::rows_per_block;

constexpr int MAX_D = 64;           // output dims
constexpr int64_t MAX_N = 50000;    // dense n x n FP64 dissimilarities: 20 GB at the cap
constexpr double ZERO_DIST = 1e-5;  // sklearn: distances[distances == 0] = 1e-5
constexpr int DIS_T = frisk_common::PAIR_T;         // dissimilarity tile (rows and columns)
constexpr int DIS_KC = frisk_common::PAIR_KC;       // input columns per LDS chunk

// ---------------------------------------------------------------------------------------------------------- dissimilarities
// pair_tile's value of a pair from its sum of squared differences: D_ij = sqrt(s)
struct Distance {
    __device__ double operator()(double s) const { return sqrt(s); }
};

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
    frisk_common::DevMem mem;
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
        hipLaunchKernelGGL((frisk_common::pair_tile<Distance, int64_t>), dim3(T, T), dim3(256), 0, 0, X, n, f, Distance(), D);
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipDeviceSynchronize());
        return 0;
    }

    // One pass from Y: stress and sum of squared distances of Y to the host (sums_out[2]); with guttman, Ynext = the next state.
    int step(const double* Y, double* Ynext, int guttman, double* sums_out) {
        const unsigned nb = unsigned(step_blocks());
        frisk_common::for_rows_per_block<MAX_D>(d, [&](auto maxd, auto r) {
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

