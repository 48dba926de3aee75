// proj_kernels.h - projection and clustering of the anomalous windows' k-mer proportions (the reference's L1597-1697):
// PCA (column mean, centring, covariance, transform), DBSCAN and Lloyd's k-means, FP64 throughout.
//
// Every reduction has a fixed order and no floating-point atomic, so every output is bit-identical from run to run:
//   column sums   per-split partials over fixed row ranges (frisk_common::colsum_part), summed split 0, 1, ... by one thread per
//                 column;
//   covariance    v_mfma_f64_16x16x4_f64 over fixed row ranges (one per split), partial tiles summed in split order;
//   transform     one wave per row, lanes over features in stride order, then a fixed xor butterfly;
//   DBSCAN        integer counts; union-find whose result does not depend on the order of the unions (see dbscan below);
//   k-means       per-block partials (fixed wave butterfly + waves in order), blocks summed in order by one thread per value;
//                 empty clusters take the farthest points by exact comparisons (descending distance, lowest index on a tie).
// Included from frisk_analysis.hip; the C entry points there are thin wrappers of the drivers below.  What the other analysis
// headers share with this one (device memory, the fixed-order sums, the column-sum kernel, the dispatches) is analysis_common.h.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "analysis_common.h"

namespace frisk_proj {

using frisk_common::block_sum;
using frisk_common::colsum_part;
using frisk_common::DevMem;
using frisk_common::for_width;
using frisk_common::round_up;
using frisk_common::RowSplits;
using frisk_common::wave_sum;

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int COV_T = 64;           // covariance output tile (4 waves of 32 x 32, each 2 x 2 MFMA tiles of 16 x 16)
constexpr int COV_KSTEP = 16;       // rows per unrolled step of the K loop; padded row count and split length are multiples
constexpr int MEAN_SPLITS = 64;     // row ranges of the column sums
constexpr int MEAN_UNROLL = 1;      // ... whose row loop is not unrolled (what the compiler does with it unasked)

// ---------------------------------------------------------------------------------------------------------- PCA
// mean[c] = (the range partials of column c, frisk_common::colsum_part, in range order) / n
__global__ __launch_bounds__(256) void proj_colmean(const double* __restrict__ part, int nsplit, int64_t n, int64_t f,
                                                    double* __restrict__ mean) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c >= f) return;
    double s = 0.0;
    for (int p = 0; p < nsplit; ++p) s += part[int64_t(p) * f + c];
    mean[c] = s / double(n);
}

// Xc[r][c] (n_pad x f_pad, zero outside n x f) = X[r][c] - mean[c]: the second pass of the two-pass centring
__global__ __launch_bounds__(256) void proj_center(const double* __restrict__ X, const double* __restrict__ mean, int64_t n,
                                                   int64_t f, int64_t n_pad, int64_t f_pad, double* __restrict__ Xc) {
    const int64_t total = n_pad * f_pad;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int64_t r = e / f_pad, c = e - r * f_pad;
        Xc[e] = (r < n && c < f) ? X[r * f + c] - mean[c] : 0.0;
    }
}

// (bi, bj), bi <= bj, of the t-th upper-triangle tile in row order
__device__ inline void upper_tile(int t, int T, int& bi, int& bj) {
    int i = 0;
    while (t >= T - i) { t -= T - i; ++i; }
    bi = i; bj = i + t;
}

// One block = one 64 x 64 tile of the upper triangle of XcT Xc over the rows of split blockIdx.y.
// v_mfma_f64_16x16x4_f64: lane l holds A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15] (one f64 each); C/D register r of lane l
// is element (row (l>>4) + 4r, col l&15).  Here A[i][k] = Xc[k][i] and B[k][j] = Xc[k][j]: both read a row of Xc.
__global__ __launch_bounds__(256) void proj_cov_part(const double* __restrict__ Xc, int64_t f_pad, int64_t n_pad, int64_t rows_per,
                                                     int T, int ntile, double* __restrict__ part) {
    int bi, bj;
    upper_tile(blockIdx.x, T, bi, bj);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane >> 4, lc = lane & 15;
    const int64_t ci = int64_t(bi) * COV_T + (wave >> 1) * 32 + lc;
    const int64_t cj = int64_t(bj) * COV_T + (wave & 1) * 32 + lc;
    const int64_t k0 = int64_t(blockIdx.y) * rows_per;
    const int64_t k1 = k0 + rows_per < n_pad ? k0 + rows_per : n_pad;
    dbl4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
    for (int64_t k = k0; k < k1; k += COV_KSTEP) {
#pragma unroll
        for (int u = 0; u < COV_KSTEP; u += 4) {
            const double* row = Xc + (k + u + lr) * f_pad;
            const double a0 = row[ci], a1 = row[ci + 16], b0 = row[cj], b1 = row[cj + 16];
            acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc11, 0, 0, 0);
        }
    }
    double* out = part + (int64_t(blockIdx.y) * ntile + blockIdx.x) * (COV_T * COV_T);
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wr + lr + 4 * r, col = wc + lc;
        out[(row) * COV_T + col] = acc00[r];
        out[(row) * COV_T + col + 16] = acc01[r];
        out[(row + 16) * COV_T + col] = acc10[r];
        out[(row + 16) * COV_T + col + 16] = acc11[r];
    }
}

// cov[i][j] = cov[j][i] = (sum of the split partials, in split order) / denom.  Diagonal tiles use their upper half only, so the
// result is exactly symmetric.
__global__ __launch_bounds__(256) void proj_cov_reduce(const double* __restrict__ part, int nsplit, int T, int ntile, int64_t f,
                                                       double denom, double* __restrict__ cov) {
    int bi, bj;
    upper_tile(blockIdx.x, T, bi, bj);
    for (int e = threadIdx.x; e < COV_T * COV_T; e += 256) {
        const int r = e / COV_T, c = e % COV_T;
        if (bi == bj && r > c) continue;
        const int64_t i = int64_t(bi) * COV_T + r, j = int64_t(bj) * COV_T + c;
        if (i >= f || j >= f) continue;
        double s = 0.0;
        for (int p = 0; p < nsplit; ++p) s += part[(int64_t(p) * ntile + blockIdx.x) * (COV_T * COV_T) + e];
        s /= denom;
        cov[i * f + j] = s;
        cov[j * f + i] = s;
    }
}

// Y[r][q] = sum_c Xc[r][c] V[c][q]: one wave per row, lane l takes features l, l + 64, ... in order
__global__ __launch_bounds__(256) void proj_transform(const double* __restrict__ Xc, const double* __restrict__ V, int64_t n,
                                                      int64_t f, int64_t f_pad, int d, double* __restrict__ Y) {
    const int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const double* row = Xc + r * f_pad;
    for (int q = 0; q < d; ++q) {
        double s = 0.0;
        for (int64_t c = lane; c < f; c += 64) s += row[c] * V[c * d + q];
        s = wave_sum(s);
        if (lane == 0) Y[r * d + q] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------- DBSCAN
// Pairs are visited through LDS tiles of the points.  A pair (i, j) is a neighbour pair when sqrt(sum_k (y_ik - y_jk)^2) <= eps,
// the squares summed in dimension order (as sklearn compares distances, so that a tie at exactly eps is a neighbour).  The
// square root is taken only for sums within a few ulps of eps^2: below lo = eps^2 (1 - 4e-15) the correctly rounded root is
// certainly <= eps, above hi = eps^2 (1 + 4e-15) certainly > eps.
enum { DB_COUNT = 0, DB_UNION = 1, DB_BORDER = 2 };

__device__ inline int32_t uf_find(int32_t* P, int32_t x) {
    for (;;) {
        const int32_t p = __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

// Hook the larger root under the smaller one.  Parents only ever decrease, so finds terminate, and the smallest index of a
// component can never be hooked: it is the component's final root whatever order the unions arrive in.
__device__ inline void uf_unite(int32_t* P, int32_t a, int32_t b) {
    for (;;) {
        a = uf_find(P, a);
        b = uf_find(P, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        int32_t expect = a;
        if (__hip_atomic_compare_exchange_strong(P + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

// MODE DB_COUNT: cnt[i] = neighbours of i, itself included.
// MODE DB_UNION: unite every core pair (j < i).
// MODE DB_BORDER: lab[i] = root of i for a core point; for any other point the smallest root among its core neighbours, or -1.
template <int MAXD, int MODE>
__global__ __launch_bounds__(256) void db_pairs(const double* __restrict__ Y, int64_t n, int d, double eps, double lo, double hi,
                                                int32_t min_samples, int32_t* __restrict__ cnt, int32_t* __restrict__ P, int32_t* __restrict__ lab) {
    constexpr int TP = 4096 / MAXD;             // points per LDS tile (32 KB)
    __shared__ double tile[TP * MAXD];
    const int64_t b0 = int64_t(blockIdx.x) * 256;
    const int64_t i = b0 + threadIdx.x;
    const bool valid = i < n;
    bool core = false;
    if (MODE != DB_COUNT && valid) core = cnt[i] >= min_samples;
    bool active = valid;
    if (MODE == DB_UNION) active = valid && core;
    if (MODE == DB_BORDER) {
        if (valid && core) lab[i] = P[i];
        active = valid && !core;
    }
    if (!__syncthreads_or(active)) return;
    double yi[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; ++k) yi[k] = (valid && k < d) ? Y[i * d + k] : 0.0;
    // unions only look at j < i: tiles past the block's last point are skipped
    const int64_t jend = MODE == DB_UNION ? (b0 + 256 < n ? b0 + 256 : n) : n;
    int32_t count = 0, best = INT32_MAX;
    for (int64_t j0 = 0; j0 < jend; j0 += TP) {
        const int64_t m = jend - j0 < TP ? jend - j0 : TP;
        __syncthreads();
        for (int64_t e = threadIdx.x; e < m * d; e += 256) tile[e] = Y[j0 * d + e];
        __syncthreads();
        if (!active) continue;
        const int64_t mm = MODE == DB_UNION ? (i - j0 < m ? i - j0 : m) : m;
        for (int64_t jj = 0; jj < mm; ++jj) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < MAXD; ++k) {
                if (k < d) {
                    const double t = yi[k] - tile[jj * d + k];
                    s += t * t;
                }
            }
            if (!(s <= lo || (s < hi && sqrt(s) <= eps))) continue;
            const int64_t j = j0 + jj;
            if (MODE == DB_COUNT) {
                ++count;
            } else if (cnt[j] >= min_samples) {
                if (MODE == DB_UNION) uf_unite(P, int32_t(i), int32_t(j));
                else { const int32_t r = P[j]; best = r < best ? r : best; }
            }
        }
    }
    if (MODE == DB_COUNT && valid) cnt[i] = count;
    if (MODE == DB_BORDER && active) lab[i] = best == INT32_MAX ? -1 : best;
}

__global__ __launch_bounds__(256) void db_init(int64_t n, int32_t* __restrict__ P) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) P[i] = int32_t(i);
}

__global__ __launch_bounds__(256) void db_compress(int64_t n, const int32_t* __restrict__ cnt, int32_t min_samples, int32_t* P) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && cnt[i] >= min_samples)
        __hip_atomic_store(P + i, uf_find(P, int32_t(i)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------- k-means
// One Lloyd step, first half: nearest centre of each point (lowest index on a tie), whether any label changed, dist[i] = the
// squared distance of point i to that centre, and per block part[b][c (d+1) + q] = sum of coordinate q (q = d: the count) of the
// block's points of centre c, part[b][k (d+1)] = their squared distances.
template <int MAXD>
__global__ __launch_bounds__(256) void km_assign(const double* __restrict__ Y, int64_t n, int d, int k, const double* __restrict__ C,
                                                 int32_t* __restrict__ lab, int32_t* __restrict__ changed, double* __restrict__ dist,
                                                 double* __restrict__ part) {
    __shared__ double red[4];
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < n;
    double yi[MAXD];
#pragma unroll
    for (int q = 0; q < MAXD; ++q) yi[q] = (valid && q < d) ? Y[i * d + q] : 0.0;
    int best = 0;
    double bd = 0.0;
    if (valid) {
        for (int c = 0; c < k; ++c) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < MAXD; ++q) {
                if (q < d) {
                    const double t = yi[q] - C[c * d + q];
                    s += t * t;
                }
            }
            if (c == 0 || s < bd) { bd = s; best = c; }
        }
        if (lab[i] != best) { lab[i] = best; *changed = 1; }
        dist[i] = bd;
    }
    const int stride = k * (d + 1) + 1;
    double* out = part + int64_t(blockIdx.x) * stride;
    for (int c = 0; c < k; ++c) {
        const bool mine = valid && best == c;
#pragma unroll
        for (int q = 0; q < MAXD + 1; ++q) {
            if (q <= d) {
                const double s = block_sum(mine ? (q < d ? yi[q] : 1.0) : 0.0, red);
                if (threadIdx.x == 0) out[c * (d + 1) + q] = s;
            }
        }
    }
    const double s = block_sum(valid ? bd : 0.0, red);
    if (threadIdx.x == 0) out[k * (d + 1)] = s;
}

// (distance, index) of the farthest point strictly after (pd, pi) in the order "descending distance, lowest index on a tie"
// (first = true: of all points), over the block: each thread scans its stride, then a wave butterfly and the waves in order.
// Exact comparisons only, so the result does not depend on the reduction order.
__device__ inline void km_farthest(const double* __restrict__ dist, int64_t n, bool first, double pd, int64_t pi, double* rd,
                                   int64_t* ri, double& od, int64_t& oi) {
    double bd = -1.0;
    int64_t bi = -1;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double v = dist[i];
        if (!first && !(v < pd || (v == pd && i > pi))) continue;
        if (v > bd) { bd = v; bi = i; }           // i increases along the stride: the first of equal distances is kept
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double od_ = __shfl_xor(bd, m, 64);
        const int64_t oi_ = __shfl_xor(bi, m, 64);
        if (oi_ >= 0 && (bi < 0 || od_ > bd || (od_ == bd && oi_ < bi))) { bd = od_; bi = oi_; }
    }
    if ((threadIdx.x & 63) == 0) { rd[threadIdx.x >> 6] = bd; ri[threadIdx.x >> 6] = bi; }
    __syncthreads();
    od = -1.0; oi = -1;
    for (int w = 0; w < 4; ++w)
        if (ri[w] >= 0 && (oi < 0 || rd[w] > od || (rd[w] == od && ri[w] < oi))) { od = rd[w]; oi = ri[w]; }
    __syncthreads();
}

// Second half (one block), sklearn's Lloyd step (lloyd_iter_chunked_dense: _relocate_empty_clusters_dense, then
// _average_centers).  S[c][q], W[c] = the block partials of coordinate sums and counts, summed in block order.  When clusters are
// empty, and the largest of the point distances dist[] is not 0, the empty clusters in increasing id take the farthest points in
// descending distance order (lowest index on a tie): each such point's coordinates and weight move out of its cluster's sums
// into the empty one's.  Then Cn[c] = S[c] / W[c]; a cluster still empty is placed where sklearn places it, on the cluster a of
// largest weight (the first of equal weights): S[a] / W[a] if a < c, else S[a] (sklearn averages in id order and copies
// whichever it finds).  res[0] = sum over centres of |Cn_c - C_c|^2 (sklearn's center_shift_tot), res[1] = the inertia of the
// assignment.  Scratch: S[k d], W[k], emp[k] (int32), far[k] (int64).
__global__ __launch_bounds__(256) void km_update(const double* __restrict__ part, int64_t nblocks, const double* __restrict__ Y,
                                                 int64_t n, int d, int k, const int32_t* __restrict__ lab,
                                                 const double* __restrict__ dist, const double* __restrict__ C, double* __restrict__ Cn,
                                                 double* __restrict__ S, double* __restrict__ W, int32_t* __restrict__ emp,
                                                 int64_t* __restrict__ far, double* __restrict__ res) {
    __shared__ double rd[4];
    __shared__ int64_t ri[4];
    __shared__ int n_empty_s, argmax_s;
    const int stride = k * (d + 1) + 1;
    for (int e = threadIdx.x; e < k * d; e += 256) {
        const int c = e / d, q = e % d;
        double s = 0.0;
        for (int64_t b = 0; b < nblocks; ++b) s += part[b * stride + c * (d + 1) + q];
        S[e] = s;
    }
    for (int c = threadIdx.x; c < k; c += 256) {
        double w = 0.0;
        for (int64_t b = 0; b < nblocks; ++b) w += part[b * stride + c * (d + 1) + d];
        W[c] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = 0;
        for (int c = 0; c < k; ++c)
            if (W[c] == 0.0) emp[m++] = c;
        n_empty_s = m;
    }
    __syncthreads();
    const int n_empty = n_empty_s;
    if (n_empty > 0) {
        double pd = 0.0;
        int64_t pi = -1;
        bool relocate = true;
        for (int t = 0; t < n_empty; ++t) {
            km_farthest(dist, n, t == 0, pd, pi, rd, ri, pd, pi);
            if (t == 0 && pd == 0.0) { relocate = false; break; }     // duplicates only: relocating is pointless (as sklearn)
            if (threadIdx.x == 0) far[t] = pi;
        }
        __syncthreads();
        if (relocate && threadIdx.x == 0) {
            for (int t = 0; t < n_empty; ++t) {
                const int nc = emp[t];
                const int64_t i = far[t];
                const int oc = lab[i];
                for (int q = 0; q < d; ++q) {
                    S[oc * d + q] -= Y[i * d + q];
                    S[nc * d + q] = Y[i * d + q];
                }
                W[nc] = 1.0;
                W[oc] -= 1.0;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int a = 0;
        for (int c = 1; c < k; ++c)
            if (W[c] > W[a]) a = c;
        argmax_s = a;
    }
    __syncthreads();
    const int a = argmax_s;
    for (int e = threadIdx.x; e < k * d; e += 256) {
        const int c = e / d, q = e % d;
        Cn[e] = W[c] > 0.0 ? S[e] / W[c] : (a < c ? S[a * d + q] / W[a] : S[a * d + q]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double shift = 0.0, inertia = 0.0;
        for (int c = 0; c < k; ++c) {
            double s = 0.0;
            for (int q = 0; q < d; ++q) { const double t = Cn[c * d + q] - C[c * d + q]; s += t * t; }
            const double norm = sqrt(s);
            shift += norm * norm;
        }
        for (int64_t b = 0; b < nblocks; ++b) inertia += part[b * stride + k * (d + 1)];
        res[0] = shift;
        res[1] = inertia;
    }
}

// ---------------------------------------------------------------------------------------------------------- host drivers
// Centred, zero-padded copy of X on the device; mean (length f) on the device.  Returns 0 or -2.
struct Centred {
    double* Xc = nullptr;
    double* mean = nullptr;
    int64_t n_pad = 0, f_pad = 0;
};

inline int upload_centred(DevMem& mem, const double* X, int64_t n, int64_t f, const double* mean_in, int64_t n_pad_mult, Centred& out) {
    out.n_pad = round_up(n, n_pad_mult);
    out.f_pad = round_up(f, COV_T);
    double* dX = mem.get<double>(size_t(n * f));
    out.Xc = mem.get<double>(size_t(out.n_pad * out.f_pad));
    out.mean = mem.get<double>(size_t(f));
    if (!dX || !out.Xc || !out.mean) return -2;
    FRISK_HIP_CHECK(hipMemcpy(dX, X, size_t(n * f) * sizeof(double), hipMemcpyHostToDevice));
    const unsigned gf = unsigned((f + 255) / 256);
    if (mean_in) {
        FRISK_HIP_CHECK(hipMemcpy(out.mean, mean_in, size_t(f) * sizeof(double), hipMemcpyHostToDevice));
    } else {
        const RowSplits sp(n, MEAN_SPLITS);
        double* part = mem.get<double>(size_t(sp.count) * size_t(f));
        if (!part) return -2;
        hipLaunchKernelGGL(colsum_part<MEAN_UNROLL>, dim3(gf, unsigned(sp.count)), dim3(256), 0, 0, dX, n, f, sp.rows_per, part);
        hipLaunchKernelGGL(proj_colmean, dim3(gf), dim3(256), 0, 0, part, int(sp.count), n, f, out.mean);
    }
    const int64_t total = out.n_pad * out.f_pad;
    const unsigned gc = unsigned(std::min<int64_t>((total + 255) / 256, 65536));
    hipLaunchKernelGGL(proj_center, dim3(gc), dim3(256), 0, 0, dX, out.mean, n, f, out.n_pad, out.f_pad, out.Xc);
    FRISK_HIP_CHECK(hipGetLastError());
    return 0;
}

// K split of the n_pad rows (a multiple of COV_KSTEP) that proj_cov_part sums per tile: enough blocks to fill the chip, a split
// length that depends on the shape only (so results are reproducible)
struct KSplit {
    int64_t nsplit, rows_per;
};
inline KSplit cov_ksplit(int64_t n_pad, int ntile) {
    int64_t nsplit = std::max<int64_t>(1, (2048 + ntile - 1) / ntile);
    nsplit = std::min<int64_t>(nsplit, n_pad / COV_KSTEP);
    const int64_t rows_per = round_up((n_pad + nsplit - 1) / nsplit, COV_KSTEP);
    return {(n_pad + rows_per - 1) / rows_per, rows_per};
}

// mean_out[f], cov_out[f*f] = XcT Xc / (n - 1) (n = 1: / 1).  Returns 0 or -2.
inline int cov(const double* X, int64_t n, int64_t f, double* mean_out, double* cov_out) {
    DevMem mem;
    Centred cx;
    if (int e = upload_centred(mem, X, n, f, nullptr, COV_KSTEP, cx)) return e;
    const int T = int(cx.f_pad / COV_T);
    const int ntile = T * (T + 1) / 2;
    const auto [nsplit, rows_per] = cov_ksplit(cx.n_pad, ntile);
    double* part = mem.get<double>(size_t(nsplit) * size_t(ntile) * COV_T * COV_T);
    double* dcov = mem.get<double>(size_t(f * f));
    if (!part || !dcov) return -2;
    hipLaunchKernelGGL(proj_cov_part, dim3(unsigned(ntile), unsigned(nsplit)), dim3(256), 0, 0, cx.Xc, cx.f_pad, cx.n_pad, rows_per, T,
                       ntile, part);
    hipLaunchKernelGGL(proj_cov_reduce, dim3(unsigned(ntile)), dim3(256), 0, 0, part, int(nsplit), T, ntile, f,
                       n > 1 ? double(n - 1) : 1.0, dcov);
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(mean_out, cx.mean, size_t(f) * sizeof(double), hipMemcpyDeviceToHost));
    FRISK_HIP_CHECK(hipMemcpy(cov_out, dcov, size_t(f * f) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// Y_out[n*d] = (X - mean) V, V f x d row-major.  Returns 0 or -2.
inline int transform(const double* X, const double* mean, const double* V, int64_t n, int64_t f, int d, double* Y_out) {
    DevMem mem;
    Centred cx;
    if (int e = upload_centred(mem, X, n, f, mean, 1, cx)) return e;
    double* dV = mem.get<double>(size_t(f) * size_t(d));
    double* dY = mem.get<double>(size_t(n) * size_t(d));
    if (!dV || !dY) return -2;
    FRISK_HIP_CHECK(hipMemcpy(dV, V, size_t(f) * size_t(d) * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(proj_transform, dim3(unsigned((n + 3) / 4)), dim3(256), 0, 0, cx.Xc, dV, n, f, cx.f_pad, d, dY);
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(Y_out, dY, size_t(n) * size_t(d) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

constexpr int MAX_DIMS = 64;        // largest point dimension of dbscan / kmeans

template <int MODE>
inline void db_launch(int d, unsigned grid, const double* Y, int64_t n, double eps, int32_t ms, int32_t* cnt, int32_t* P, int32_t* lab) {
    const double lo = eps * eps * (1.0 - 4e-15), hi = eps * eps * (1.0 + 4e-15);
    for_width<4, 16, MAX_DIMS>(d, [&](auto maxd) {
        hipLaunchKernelGGL((db_pairs<decltype(maxd)::value, MODE>), dim3(grid), dim3(256), 0, 0, Y, n, d, eps, lo, hi, ms, cnt, P, lab);
    });
}

// labels_out[n]: cluster ids 0, 1, ... in increasing order of their smallest core index; -1 = noise.  Returns 0 or -2.
inline int dbscan(const double* Y, int64_t n, int d, double eps, int32_t min_samples, int32_t* labels_out) {
    DevMem mem;
    double* dY = mem.get<double>(size_t(n) * size_t(d));
    int32_t* cnt = mem.get<int32_t>(size_t(n));
    int32_t* P = mem.get<int32_t>(size_t(n));
    int32_t* lab = mem.get<int32_t>(size_t(n));
    if (!dY || !cnt || !P || !lab) return -2;
    FRISK_HIP_CHECK(hipMemcpy(dY, Y, size_t(n) * size_t(d) * sizeof(double), hipMemcpyHostToDevice));
    const unsigned grid = unsigned((n + 255) / 256);
    hipLaunchKernelGGL(db_init, dim3(grid), dim3(256), 0, 0, n, P);
    db_launch<DB_COUNT>(d, grid, dY, n, eps, min_samples, cnt, P, lab);
    db_launch<DB_UNION>(d, grid, dY, n, eps, min_samples, cnt, P, lab);
    hipLaunchKernelGGL(db_compress, dim3(grid), dim3(256), 0, 0, n, cnt, min_samples, P);
    db_launch<DB_BORDER>(d, grid, dY, n, eps, min_samples, cnt, P, lab);
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(labels_out, lab, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    // a root is the smallest core index of its cluster: number the roots in index order
    std::vector<int32_t> id(size_t(n), -1);
    int32_t next = 0;
    for (int64_t i = 0; i < n; ++i)
        if (labels_out[i] == i) id[size_t(i)] = next++;
    for (int64_t i = 0; i < n; ++i)
        if (labels_out[i] >= 0) labels_out[i] = id[size_t(labels_out[i])];
    return 0;
}

// Lloyd's algorithm from init_centers, stopped as sklearn stops it: labels unchanged, or center shift <= tol, or max_iter steps.
// Then the points are assigned once more to the final centres, and the inertia is that assignment's.  Returns 0 or -2.
inline int kmeans(const double* Y, int64_t n, int d, int k, const double* init_centers, int32_t max_iter, double tol,
                  int32_t* labels_out, double* centers_out, double* inertia_out, int32_t* n_iter_out) {
    DevMem mem;
    const int64_t nblocks = (n + 255) / 256;
    const int stride = k * (d + 1) + 1;
    double* dY = mem.get<double>(size_t(n) * size_t(d));
    double* C = mem.get<double>(size_t(k) * size_t(d));
    double* Cn = mem.get<double>(size_t(k) * size_t(d));
    double* part = mem.get<double>(size_t(nblocks) * size_t(stride));
    double* res = mem.get<double>(2);
    int32_t* lab = mem.get<int32_t>(size_t(n));
    int32_t* changed = mem.get<int32_t>(1);
    double* dist = mem.get<double>(size_t(n));
    double* S = mem.get<double>(size_t(k) * size_t(d));
    double* W = mem.get<double>(size_t(k));
    int32_t* emp = mem.get<int32_t>(size_t(k));
    int64_t* far = mem.get<int64_t>(size_t(k));
    if (!dY || !C || !Cn || !part || !res || !lab || !changed || !dist || !S || !W || !emp || !far) return -2;
    FRISK_HIP_CHECK(hipMemcpy(dY, Y, size_t(n) * size_t(d) * sizeof(double), hipMemcpyHostToDevice));
    FRISK_HIP_CHECK(hipMemcpy(C, init_centers, size_t(k) * size_t(d) * sizeof(double), hipMemcpyHostToDevice));
    FRISK_HIP_CHECK(hipMemset(lab, 0xff, size_t(n) * sizeof(int32_t)));          // -1: every label changes in the first step
    auto step = [&](double* from, double* to) {
        for_width<4, 16, MAX_DIMS>(d, [&](auto maxd) {
            hipLaunchKernelGGL(km_assign<decltype(maxd)::value>, dim3(unsigned(nblocks)), dim3(256), 0, 0, dY, n, d, k, from, lab, changed,
                               dist, part);
        });
        hipLaunchKernelGGL(km_update, dim3(1), dim3(256), 0, 0, part, nblocks, dY, n, d, k, lab, dist, from, to, S, W, emp, far, res);
    };
    int32_t it = 0;
    double h[2];
    int32_t ch = 0;
    for (it = 0; it < max_iter; ++it) {
        FRISK_HIP_CHECK(hipMemset(changed, 0, sizeof(int32_t)));
        step(C, Cn);
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipMemcpy(h, res, sizeof(h), hipMemcpyDeviceToHost));
        FRISK_HIP_CHECK(hipMemcpy(&ch, changed, sizeof(ch), hipMemcpyDeviceToHost));
        std::swap(C, Cn);
        if (!ch || h[0] <= tol) break;
    }
    const int32_t iters = it < max_iter ? it + 1 : max_iter;
    step(C, Cn);                    // final assignment to the final centres (Cn is scratch here)
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(h, res, sizeof(h), hipMemcpyDeviceToHost));
    FRISK_HIP_CHECK(hipMemcpy(labels_out, lab, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    FRISK_HIP_CHECK(hipMemcpy(centers_out, C, size_t(k) * size_t(d) * sizeof(double), hipMemcpyDeviceToHost));
    if (inertia_out) *inertia_out = h[1];
    if (n_iter_out) *n_iter_out = iters;
    return 0;
}


}  // namespace frisk_proj
