// spectral_kernels.h - the dense n x n work of spectral clustering as the reference's --cluster SPECTRAL runs it (sklearn.cluster.
// SpectralClustering(affinity='rbf', gamma, assign_labels='kmeans'): pairwise_kernels 'rbf', scipy.sparse.csgraph.laplacian(normed=
// True), then the top eigenvectors of M = D^-1/2 A0 D^-1/2), FP64.
//
// Layout (n points, d <= 64 dims): ONE n x n buffer, which holds the affinities A0 and is then normalised in place to M.  Every
// reduction has a fixed order that depends on the shape only, and there is no floating-point atomic: every output is bit-identical
// from run to run.
//   affinity   A0_ij = exp(-gamma sum_c (y_ic - y_jc)^2), c in order, by direct differences (the Gram form cancels for close
//              pairs): 64 x 64 tiles of the upper triangle, the columns of Y streamed through LDS in chunks of AFF_KC, each
//              thread a 4 x 4 micro-tile; the tile and its mirror are written from the same values, so A0 is exactly symmetric, and
//              the diagonal is exactly 0 (scipy drops it).
//   degrees    w_j = sum_i A0_ij: one lane per column, the rows in `splits` contiguous ranges, each in row order
//              (colsum_part); the ranges summed in range order, w == 0 replaced by 1 and counted, dd = sqrt(w) (spec_degrees).
//   normalise  scipy divides twice, m /= dd (per column) then m /= dd[:, None] (per row): r = (A0_ij / dd_j) / dd_i.  Its mirror
//              entry is r' = (A0_ji / dd_i) / dd_j, the same value but for the last two roundings, up to 2 ulps away.  Every entry is
//              written as (r + r') / 2, which is symmetric in (i, j), lies between r and r', and is r itself wherever r' == r: M is
//              exactly symmetric and each half is within 1 ulp of scipy's entry.
//   Z = M Q    (n x p, p <= SPECTRAL_MAX_P): one wave per R rows, lane l takes columns l, l + 64, ... in order, then a wave
//              butterfly - the order of frisk_nmf_impl::nmf_xq, and the same bits - with Q staged through LDS per block.  Plain
//              VALU: bound by reading M once (DESIGN.md section 9.5 has the measured fraction of the HBM rate).
// The eigen-iteration itself (QR and Rayleigh-Ritz on matrices at most 26 wide) is the host's: frisk_amd/projection.py.
// Included from frisk_analysis.hip after nmf_kernels.h; the C entry points there are thin wrappers of the driver below.  The tile
// kernel of the affinities (pair_tile, shared with MDS), the column sums of the degrees (colsum_part, shared with PCA), wave_sum,
// the row split, the width dispatch and the event timer are analysis_common.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "analysis_common.h"

namespace frisk_spectral_impl {

constexpr int64_t MAX_N = 50000;        // the dense n x n FP64 buffer: 20 GB at the cap
constexpr int SPECTRAL_MAX_K = 16;      // clusters = eigenvectors
constexpr int SPECTRAL_MAX_P = 26;      // columns of a product: k plus the 10 guard columns of the subspace iteration
constexpr int AFF_T = frisk_common::PAIR_T;         // affinity tile (rows and columns)
constexpr int AFF_KC = frisk_common::PAIR_KC;       // columns of Y per LDS chunk
constexpr int DEG_SPLITS = 256;         // most row ranges of the column sums
constexpr int DEG_MIN_ROWS = 32;        // fewest rows per range (but for the last)
constexpr int DEG_UNROLL = 4;           // rows per unrolled step of a range's sum

// ---------------------------------------------------------------------------------------------------------- affinity
// pair_tile's value of a pair from its sum of squared differences: sklearn's K *= -gamma; exp(K)
struct Rbf {
    double minus_gamma;
    __device__ double operator()(double s) const { return exp(minus_gamma * s); }
};

// ---------------------------------------------------------------------------------------------------------- degrees
// w_j = the range partials of column j (frisk_common::colsum_part over A0, n x n) in range order; w == 0 -> 1 (scipy's isolated
// node), counted in *n_isolated (an integer atomic: exact in any order); dd_j = sqrt(w_j).
__global__ __launch_bounds__(256) void spec_degrees(const double* __restrict__ part, int nsplit, int64_t n, double* __restrict__ dd,
                                                    unsigned long long* __restrict__ n_isolated) {
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= n) return;
    double w = 0.0;
    for (int k = 0; k < nsplit; ++k) w += part[int64_t(k) * n + j];
    if (w == 0.0) {
        w = 1.0;
        atomicAdd(n_isolated, 1ull);
    }
    dd[j] = sqrt(w);
}

// ---------------------------------------------------------------------------------------------------------- normalise
// In place, one thread per entry: A_ij <- ((A_ij / dd_j) / dd_i + (A_ij / dd_i) / dd_j) / 2.  A is exactly symmetric on entry, so
// entry (j, i) computes the same two quotients and the same sum.
__global__ __launch_bounds__(256) void spec_normalise(double* __restrict__ A, const double* __restrict__ dd, int64_t n) {
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j >= n) return;
    const double a = A[i * n + j], di = dd[i], dj = dd[j];
    const double r = (a / dj) / di;             // scipy's entry (i, j)
    const double rt = (a / di) / dj;            // scipy's entry (j, i)
    A[i * n + j] = 0.5 * (r + rt);
}

// ---------------------------------------------------------------------------------------------------------- Z = M Q
// Wave w of block b owns rows (4 b + w) R .. + R - 1; lane l takes columns l, l + 64, ... in order, each row's p sums then go
// through the wave butterfly: the summation order of frisk_nmf_impl::nmf_xq, so the same bits.  What differs is where Q comes
// from: nmf_xq has every lane read its p values of Q from global memory for every 64 columns of every wave (p x the bytes of M,
// out of L2); here the block stages MQ_C rows of Q in LDS once, transposed (Qs[q][column]: a wave reads 64 consecutive doubles),
// and its four waves share them.  Columns q >= p of Qs stay zero.
constexpr int MQ_C = 128;               // columns of M (rows of Q) per LDS stage: two per lane

template <int PMAX, int R>
__global__ __launch_bounds__(256, 2) void spec_mq(const double* __restrict__ M, const double* __restrict__ Q, int64_t n, int p,
                                               double* __restrict__ Z) {
    __shared__ double Qs[PMAX][MQ_C + 2];               // + 2: the staging writes of one column's p values spread over the banks
    const int lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * R;
    for (int e = threadIdx.x; e < PMAX * MQ_C; e += 256) Qs[e / MQ_C][e % MQ_C] = 0.0;
    const int q_first = int(threadIdx.x) % p, col_first = int(threadIdx.x) / p;        // entry e = col p + q of a stage; e += 256
    const int q_step = 256 % p, col_step = 256 / p;
    double acc[R][PMAX];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int q = 0; q < PMAX; ++q) acc[a][q] = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += MQ_C) {
        double x[MQ_C / 64][R];                             // this stage's entries of M, asked for before Q is staged
#pragma unroll
        for (int h = 0; h < MQ_C / 64; ++h) {
            const int64_t c = c0 + 64 * h + lane;
#pragma unroll
            for (int a = 0; a < R; ++a) x[h][a] = (c < n && r0 + a < n) ? M[(r0 + a) * n + c] : 0.0;
        }
        __syncthreads();                                    // the stage before this one has been read (first: the zeros are in)
        const int cols = int(n - c0 < MQ_C ? n - c0 : MQ_C);
        const double* Qc = Q + c0 * p;                      // the stage's rows of Q are contiguous: coalesced
        for (int e = threadIdx.x, q = q_first, col = col_first; col < MQ_C; e += 256) {
            Qs[q][col] = col < cols ? Qc[e] : 0.0;          // beyond n (the last stage): zeros, nothing stale
            q += q_step;
            col += col_step;
            if (q >= p) {
                q -= p;
                ++col;
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < MQ_C / 64; ++h) {
#pragma unroll
            for (int q = 0; q < PMAX; ++q) {
                const double qv = Qs[q][64 * h + lane];
#pragma unroll
                for (int a = 0; a < R; ++a) acc[a][q] += x[h][a] * qv;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < R; ++a) {
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            if (r0 + a < n && q < p) {                      // uniform over the wave
                const double s = frisk_common::wave_sum(acc[a][q]);
                if (lane == 0) Z[(r0 + a) * p + q] = s;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- host driver
// Device state of one problem (the C handle frisk_spectral).  Every buffer is allocated by create.
struct State {
    int device = 0;
    int64_t n = 0;
    int d = 0;
    double gamma = 1.0;
    int64_t n_isolated = 0;
    frisk_common::DevMem mem;
    double *Y = nullptr, *A = nullptr, *dd = nullptr, *part = nullptr, *Q = nullptr, *Z = nullptr;
    unsigned long long* iso = nullptr;
    frisk_common::EventTimer<2> timer;
    double ms[3] = {0.0, 0.0, 0.0};     // of the last call of each kind: affinity, degrees + normalise, a product

    frisk_common::RowSplits splits() const { return {n, DEG_SPLITS, DEG_MIN_ROWS}; }

    // A <- A0 of Y
    int launch_affinity() {
        const unsigned T = unsigned((n + AFF_T - 1) / AFF_T);
        FRISK_HIP_CHECK(timer.record(0));
        hipLaunchKernelGGL((frisk_common::pair_tile<Rbf, int>), dim3(T, T), dim3(256), 0, 0, Y, n, d, Rbf{-gamma}, A);
        FRISK_HIP_CHECK(timer.record(1));
        FRISK_HIP_CHECK(hipGetLastError());
        return timer.elapsed(0, 1, ms[0]);
    }

    // A0 -> M in place; with_degrees: dd and the isolated count from A0 first (they are kept for the life of the handle)
    int launch_normalise(bool with_degrees) {
        const unsigned gx = unsigned((n + 255) / 256);
        FRISK_HIP_CHECK(timer.record(0));
        if (with_degrees) {
            FRISK_HIP_CHECK(hipMemsetAsync(iso, 0, sizeof(unsigned long long), 0));
            const frisk_common::RowSplits sp = splits();
            hipLaunchKernelGGL(frisk_common::colsum_part<DEG_UNROLL>, dim3(gx, unsigned(sp.count)), dim3(256), 0, 0, A, n, n, sp.rows_per,
                               part);
            hipLaunchKernelGGL(spec_degrees, dim3(gx), dim3(256), 0, 0, part, int(sp.count), n, dd, iso);
        }
        hipLaunchKernelGGL(spec_normalise, dim3(gx, unsigned(n)), dim3(256), 0, 0, A, dd, n);
        FRISK_HIP_CHECK(timer.record(1));
        FRISK_HIP_CHECK(hipGetLastError());
        if (with_degrees) {
            unsigned long long c = 0;
            FRISK_HIP_CHECK(hipMemcpy(&c, iso, sizeof(c), hipMemcpyDeviceToHost));
            n_isolated = int64_t(c);
            return timer.elapsed(0, 1, ms[1]);
        }
        FRISK_HIP_CHECK(hipDeviceSynchronize());
        return 0;
    }

    // Allocates everything and leaves M in the buffer.  Returns 0 or -2.
    int create(const double* Y_in) {
        const size_t sn = size_t(n);
        A = mem.get<double>(sn * sn);
        Y = mem.get<double>(sn * size_t(d));
        dd = mem.get<double>(sn);
        part = mem.get<double>(size_t(splits().count) * sn);
        Q = mem.get<double>(sn * SPECTRAL_MAX_P);
        Z = mem.get<double>(sn * SPECTRAL_MAX_P);
        iso = mem.get<unsigned long long>(1);
        if (!A || !Y || !dd || !part || !Q || !Z || !iso) return -2;
        if (timer.create()) return -2;
        FRISK_HIP_CHECK(hipMemcpy(Y, Y_in, sn * size_t(d) * sizeof(double), hipMemcpyHostToDevice));
        if (launch_affinity()) return -2;
        return launch_normalise(true);
    }

    // A0_out[n][n]: the affinities again (same kernel, same bits), then M restored from the kept dd
    int affinity(double* A0_out) {
        if (launch_affinity()) return -2;
        FRISK_HIP_CHECK(hipMemcpy(A0_out, A, size_t(n) * size_t(n) * sizeof(double), hipMemcpyDeviceToHost));
        return launch_normalise(false);
    }

    // Z_out[n][p] = M Q_in[n][p] (host buffers)
    int mq(const double* Q_in, int p, double* Z_out) {
        FRISK_HIP_CHECK(hipMemcpy(Q, Q_in, size_t(n) * size_t(p) * sizeof(double), hipMemcpyHostToDevice));
        FRISK_HIP_CHECK(timer.record(0));
        frisk_common::for_width<4, 8, 16, SPECTRAL_MAX_P>(p, [&](auto pmax) {
            constexpr int PMAX = decltype(pmax)::value, R = PMAX <= 16 ? 4 : 2;         // rows per wave
            hipLaunchKernelGGL((spec_mq<PMAX, R>), dim3(unsigned((n + 4 * R - 1) / (4 * R))), dim3(256), 0, 0, A, Q, n, p, Z);
        });
        FRISK_HIP_CHECK(timer.record(1));
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipMemcpy(Z_out, Z, size_t(n) * size_t(p) * sizeof(double), hipMemcpyDeviceToHost));
        return timer.elapsed(0, 1, ms[2]);
    }
};

}  // namespace frisk_spectral_impl
