// analysis_common.h - what the analysis headers share (proj, tsne, mds, ipca, nmf, spectral and hmm _kernels.h): the host pieces
// of a driver (error check, device memory, device switch, event timer, row-range split, width dispatch), the fixed-order sums of a
// wave and of a block, and the two kernels that more than one method launches (column sums over row ranges, pairwise 64 x 64 tiles).
// One definition each: a method that needs the bits of another gets them by calling the same code.  Included by every
// *_kernels.h of frisk_analysis.hip; nothing of the scan is included here.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

// every host driver of the analysis headers returns 0 or -2 (a HIP call failed)
#define FRISK_HIP_CHECK(call)                               \
    do {                                                    \
        if ((call) != hipSuccess) return -2;                \
    } while (0)

namespace frisk_common {

// ---------------------------------------------------------------------------------------------------------- host pieces
// Device memory of one call or one handle, freed on every return path.
struct DevMem {
    std::vector<void*> ptrs;
    ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T>
    T* get(size_t count) {
        void* p = nullptr;
        if (hipMalloc(&p, (count ? count : 1) * sizeof(T)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return static_cast<T*>(p);
    }
};

// A device buffer that grows and is never shrunk; freed with its owner.
struct Buf {
    double* p = nullptr;
    size_t cap = 0;
    ~Buf() { if (p) (void)hipFree(p); }
    double* ensure(size_t count) {
        if (count <= cap) return p;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        void* q = nullptr;
        if (hipMalloc(&q, (count ? count : 1) * sizeof(double)) != hipSuccess) return nullptr;
        p = static_cast<double*>(q);
        cap = count;
        return p;
    }
};

// The calling thread's current device is restored on return.
struct OnDevice {
    int prev = -1;
    bool ok = false;
    explicit OnDevice(int device) {
        int ndev = 0;
        if (hipGetDevice(&prev) != hipSuccess || hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~OnDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// N events on the null stream, owned by a handle's state: record(i) marks a point, elapsed(a, b, ms) is the time between two.
template <int N>
struct EventTimer {
    hipEvent_t ev[N] = {};
    ~EventTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int create() {
        for (hipEvent_t& e : ev) FRISK_HIP_CHECK(hipEventCreate(&e));
        return 0;
    }
    hipError_t record(int i) { return hipEventRecord(ev[i], 0); }
    // ms = milliseconds from event a to event b, once b has been reached (no wait where a blocking copy followed it).  0 or -2.
    int elapsed(int a, int b, double& ms) {
        float t = 0.f;
        FRISK_HIP_CHECK(hipEventSynchronize(ev[b]));
        FRISK_HIP_CHECK(hipEventElapsedTime(&t, ev[a], ev[b]));
        ms = double(t);
        return 0;
    }
};

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// dst[cols][rows] = the transpose of src[rows][cols], on the host (H and Vt arrive as [d][f]; the kernels read [f][d])
inline void transpose(const double* src, int64_t rows, int64_t cols, double* dst) {
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) dst[size_t(c) * size_t(rows) + size_t(r)] = src[size_t(r) * size_t(cols) + size_t(c)];
}

// `rows` cut into contiguous ranges of rows_per rows (the last may be shorter): at most max_splits of them, and at least min_rows
// rows in each but the last.  It depends on the shape only, so a sum over the ranges has the same order on every run.
struct RowSplits {
    int64_t rows_per, count;
    RowSplits(int64_t rows, int64_t max_splits, int64_t min_rows = 1) {
        const int64_t most = std::min<int64_t>(max_splits, (rows + min_rows - 1) / min_rows);
        rows_per = (rows + most - 1) / most;
        count = (rows + rows_per - 1) / rows_per;
    }
};

// f(std::integral_constant<int, W>) for the first W of the list with v <= W (the last W takes whatever is left): the narrowest
// instantiation of a kernel that holds a runtime width.  What depends on W is a constexpr inside f.
template <int W0, int... Ws, typename F>
inline void for_width(int v, F&& f) {
    if constexpr (sizeof...(Ws) == 0) f(std::integral_constant<int, W0>());
    else if (v <= W0) f(std::integral_constant<int, W0>());
    else for_width<Ws...>(v, f);
}

// ---------------------------------------------------------------------------------------------------------- sums
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// sum of v over a block of WAVES waves, in a fixed order: xor butterfly inside each wave, then the waves in order
template <int WAVES = 4>
__device__ inline double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w];
    __syncthreads();
    return s;
}

// ---------------------------------------------------------------------------------------------------------- rows of a block
// Rows i0 .. i0 + R - 1 of a block in LDS, zero beyond n and beyond d (t-SNE's passes, MDS's step: each thread then takes the
// points j = tid, tid + 256, ... in order).
template <int MAXD, int R>
__device__ inline void load_rows(const double* __restrict__ Y, int64_t n, int d, int64_t i0, double (*yi)[MAXD]) {
    for (int e = threadIdx.x; e < R * MAXD; e += 256) {
        const int r = e / MAXD, k = e % MAXD;
        yi[r][k] = (i0 + r < n && k < d) ? Y[(i0 + r) * d + k] : 0.0;
    }
    __syncthreads();
}
// ... how many rows that is at output dimension d, and the instantiation that goes with it: f(MAXD, R) as integral constants
constexpr int rows_per_block(int d) { return d <= 4 ? 8 : d <= 16 ? 2 : 1; }
template <int MAX_D, typename F>
inline void for_rows_per_block(int d, F&& f) {
    for_width<4, 16, MAX_D>(d, [&](auto maxd) { f(maxd, std::integral_constant<int, rows_per_block(decltype(maxd)::value)>()); });
}

// ---------------------------------------------------------------------------------------------------------- column sums
// part[s][c] = sum of X[r][c] (n x f) over the rows r of range s, in row order.  Block (bx, s): columns 256 bx .. 256 bx + 255.
// UNROLL is the row loop's unroll count (1: none), each caller's own; the order of the sum does not depend on it.
template <int UNROLL>
__global__ __launch_bounds__(256) void colsum_part(const double* __restrict__ X, int64_t n, int64_t f, int64_t rows_per,
                                                   double* __restrict__ part) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c >= f) return;
    const int64_t r0 = int64_t(blockIdx.y) * rows_per;
    const int64_t r1 = r0 + rows_per < n ? r0 + rows_per : n;
    double s = 0.0;
#pragma unroll UNROLL
    for (int64_t r = r0; r < r1; ++r) s += X[r * f + c];
    part[int64_t(blockIdx.y) * f + c] = s;
}

// ---------------------------------------------------------------------------------------------------------- pairwise tiles
constexpr int PAIR_T = 64;          // tile (rows and columns)
constexpr int PAIR_KC = 16;         // columns of X per LDS chunk

// D[i][j] = D[j][i] = epi(sum_k (x_ik - x_jk)^2), k in order, by direct differences (the Gram form cancels for close pairs); the
// diagonal is exactly 0.  X is n x f (W: the type the caller holds f in).  Block (bx, by), bx >= by, 256 threads: the tile of rows
// r0 = 64 by, columns c0 = 64 bx, f streamed through LDS in chunks of PAIR_KC columns.  Thread (ty, tx) = (tid / 16, tid % 16) owns
// rows r0 + ty + 16 a and columns c0 + tx + 16 b (a, b < 4).  The values are written to D[r][c] and D[c][r] through one LDS
// transpose, so both halves come from the same value: D is exactly symmetric.
template <typename Epi, typename W>
__global__ __launch_bounds__(256) void pair_tile(const double* __restrict__ X, int64_t n, W f, Epi epi, double* __restrict__ D) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double A[PAIR_KC][PAIR_T + 1], B[PAIR_KC][PAIR_T + 1];
    __shared__ double T[PAIR_T][PAIR_T + 1];
    const int64_t r0 = int64_t(blockIdx.y) * PAIR_T, c0 = int64_t(blockIdx.x) * PAIR_T;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double s[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) s[a][b] = 0.0;
    for (W k0 = 0; k0 < f; k0 += PAIR_KC) {
        for (int e = threadIdx.x; e < PAIR_T * PAIR_KC; e += 256) {
            const int r = e / PAIR_KC, k = e % PAIR_KC;
            const bool kin = k0 + k < f;
            A[k][r] = (kin && r0 + r < n) ? X[(r0 + r) * f + k0 + k] : 0.0;
            B[k][r] = (kin && c0 + r < n) ? X[(c0 + r) * f + k0 + k] : 0.0;
        }
        __syncthreads();
        const int kc = int(f - k0 < PAIR_KC ? f - k0 : PAIR_KC);
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
            T[u][v] = (r0 + u == c0 + v) ? 0.0 : epi(s[a][b]);
        }
    __syncthreads();
    for (int e = threadIdx.x; e < PAIR_T * PAIR_T; e += 256) {
        const int u = e / PAIR_T, v = e % PAIR_T;
        if (r0 + u < n && c0 + v < n) D[(r0 + u) * n + c0 + v] = T[u][v];       // the tile, row by row
        if (c0 + u < n && r0 + v < n) D[(c0 + u) * n + r0 + v] = T[v][u];       // its mirror, row by row
    }
}

}  // namespace frisk_common
