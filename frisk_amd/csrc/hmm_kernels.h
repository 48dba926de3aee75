// hmm_kernels.h - the 2-state Gaussian HMM of hmm_host.h on the device (FP64 throughout): Baum-Welch and Viterbi for the fine
// track of --updateHMM, whose 6.6 M windows at GRCh38 scale the host form would segment several times slower than they are
// scored.  The model and its arithmetic are those of frisk_amd/hmm.py (the specification) and hmm_host.h:
//   * deterministic 2-means start from the extremes, shared variance, flat start and transitions;
//   * E step in scaled space: the two emission densities divided by the larger one, forward / backward vectors renormalised at
//     every step, posteriors and transition posteriors normalised per window;
//   * M step with hmmlearn's default priors; the stop rule `ll - prev < tol` is evaluated in double on the host, once per round,
//     and the parameters of the round that met it are kept.
// The recursions are products of 2 x 2 matrices (associative), done in three passes: the sequence is cut into a number of pieces
// that depends on n alone (never on the grid or the CU count, so neither does the rounding), one thread forms one piece's product;
// one short serial pass resolves the vector at every cut (forward on one wave, backward on another); the pieces are walked again,
// one thread each.  The product of a piece's steps serves both directions: alpha crosses it as a row vector, beta as a column.
// Sufficient statistics (sum gamma, sum gamma x, sum gamma (x - mu)^2, sum xi, log-likelihood) are per-piece partial sums added
// in a fixed order by one block: no floating-point atomics, bit-identical from run to run.
// Viterbi is the same scheme in max-plus form, per scaffold: pieces of VIT_STEPS windows; a piece computes the best score and the
// backpointers for BOTH entry states; one thread per scaffold resolves the cuts serially (scores kept relative to the better
// state, so their magnitude - and rounding - does not grow with the scaffold); the pieces are backtracked in parallel.  Ties go
// to the lower state, as numpy.argmax.  A scaffold of at most VIT_STEPS windows is one piece, computed operation for operation
// as hmm_host.h does.
// One thread walks one piece serially: 16 bytes of state per step, latency bound; neighbouring lanes read addresses a piece
// apart, which the caches absorb (a piece is a few KiB).  Not measured against a tiled (LDS-transposed) layout.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "hmm_host.h"
#include "analysis_common.h"    // DevMem, FRISK_HIP_CHECK

namespace frisk_hmm_gpu {

constexpr int PIECES = 16384;          // fixed upper piece count of the E step: 256 waves of one piece per lane
constexpr int MIN_STEPS = 32;          // a piece has at least this many windows (so short tracks keep the serial pass short)
constexpr int VIT_STEPS = 256;         // windows per Viterbi piece
constexpr int PARTS = 1024;            // fixed upper chunk count of the start's reductions
constexpr int ACC = 10;                // per-piece sums: gamma0 gamma1 gx0 gx1 xi00 xi01 xi10 xi11 ll(emissions) ll(scales)
constexpr int RED_T = 256;

inline int pieces_of(int64_t n) { return int(std::min<int64_t>(PIECES, std::max<int64_t>(1, n / MIN_STEPS))); }
inline int parts_of(int64_t n) { return int(std::min<int64_t>(PARTS, std::max<int64_t>(1, n / RED_T))); }

struct Par {                            // one round's model, by value
    double mu0, mu1, lc0, lc1, ic0, ic1, a00, a01, a10, a11, pi0, pi1;
};

// ---------------------------------------------------------------------------------------------------- fixed-order reductions
// out[k] = sum over rows r of acc[r * K + k]: thread t adds rows t, t + 256, ... in order, then a tree over the 256 threads.
__global__ void __launch_bounds__(RED_T) hmm_reduce_rows(const double* __restrict__ acc, int rows, int K, double* __restrict__ out) {
    __shared__ double sh[RED_T];
    const int tid = threadIdx.x;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int r = tid; r < rows; r += RED_T) s += acc[size_t(r) * K + k];
        sh[tid] = s;
        __syncthreads();
        for (int h = RED_T / 2; h > 0; h >>= 1) {
            if (tid < h) sh[tid] += sh[tid + h];
            __syncthreads();
        }
        if (tid == 0) out[k] = sh[0];
        __syncthreads();
    }
}

template <int K>
__device__ inline void block_sum(double (&v)[K], double* sh, double* out) {
    const int tid = threadIdx.x;
    for (int k = 0; k < K; ++k) {
        sh[tid] = v[k];
        __syncthreads();
        for (int h = RED_T / 2; h > 0; h >>= 1) {
            if (tid < h) sh[tid] += sh[tid + h];
            __syncthreads();
        }
        if (tid == 0) out[k] = sh[0];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------- start
// chunk c of C covers [n c / C, n (c + 1) / C); part[c * 4 + {0, 1, 2}] = min, max, sum
__global__ void __launch_bounds__(RED_T) hmm_init_range(const double* __restrict__ x, int64_t n, int C, double* __restrict__ part) {
    __shared__ double sh[RED_T];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= C) return;
    const int64_t a = n * c / C, b = n * (c + 1) / C;
    double lo = std::numeric_limits<double>::infinity(), hi = -std::numeric_limits<double>::infinity(), s = 0.0;
    for (int64_t t = a + tid; t < b; t += RED_T) { const double v = x[t]; lo = fmin(lo, v); hi = fmax(hi, v); s += v; }
    double sum[1] = {s};
    block_sum<1>(sum, sh, part + size_t(c) * 4 + 2);
    sh[tid] = lo;
    __syncthreads();
    for (int h = RED_T / 2; h > 0; h >>= 1) { if (tid < h) sh[tid] = fmin(sh[tid], sh[tid + h]); __syncthreads(); }
    if (tid == 0) part[size_t(c) * 4] = sh[0];
    __syncthreads();
    sh[tid] = hi;
    __syncthreads();
    for (int h = RED_T / 2; h > 0; h >>= 1) { if (tid < h) sh[tid] = fmax(sh[tid], sh[tid + h]); __syncthreads(); }
    if (tid == 0) part[size_t(c) * 4 + 1] = sh[0];
}

// out[0..2] = min, max, sum over the chunks
__global__ void __launch_bounds__(RED_T) hmm_init_range_final(const double* __restrict__ part, int C, double* __restrict__ out) {
    __shared__ double sh[RED_T];
    const int tid = threadIdx.x;
    double lo = std::numeric_limits<double>::infinity(), hi = -std::numeric_limits<double>::infinity(), s = 0.0;
    for (int c = tid; c < C; c += RED_T) { lo = fmin(lo, part[size_t(c) * 4]); hi = fmax(hi, part[size_t(c) * 4 + 1]); s += part[size_t(c) * 4 + 2]; }
    double sum[1] = {s};
    block_sum<1>(sum, sh, out + 2);
    sh[tid] = lo;
    __syncthreads();
    for (int h = RED_T / 2; h > 0; h >>= 1) { if (tid < h) sh[tid] = fmin(sh[tid], sh[tid + h]); __syncthreads(); }
    if (tid == 0) out[0] = sh[0];
    __syncthreads();
    sh[tid] = hi;
    __syncthreads();
    for (int h = RED_T / 2; h > 0; h >>= 1) { if (tid < h) sh[tid] = fmax(sh[tid], sh[tid + h]); __syncthreads(); }
    if (tid == 0) out[1] = sh[0];
}

// one 2-means assignment: part[c * 4 + ..] = sum and count of the windows nearer c0 (ties to it, as argmin), then of the others
__global__ void __launch_bounds__(RED_T) hmm_init_assign(const double* __restrict__ x, int64_t n, int C, double c0, double c1,
                                                         double* __restrict__ part) {
    __shared__ double sh[RED_T];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= C) return;
    const int64_t a = n * c / C, b = n * (c + 1) / C;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = a + tid; t < b; t += RED_T) {
        const double xt = x[t];
        if (fabs(xt - c0) <= fabs(xt - c1)) { v[0] += xt; v[1] += 1.0; }
        else { v[2] += xt; v[3] += 1.0; }
    }
    block_sum<4>(v, sh, part + size_t(c) * 4);
}

// part[c] = sum of (x - mu)^2
__global__ void __launch_bounds__(RED_T) hmm_init_var(const double* __restrict__ x, int64_t n, int C, double mu, double* __restrict__ part) {
    __shared__ double sh[RED_T];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= C) return;
    const int64_t a = n * c / C, b = n * (c + 1) / C;
    double v[1] = {0.0};
    for (int64_t t = a + tid; t < b; t += RED_T) { const double d = x[t] - mu; v[0] += d * d; }
    block_sum<1>(v, sh, part + c);
}

// ------------------------------------------------------------------------------------------------------------------ E step
// 1. scaled emissions of every window and the normalised product of every piece's steps, S_t = A diag(b_t)
__global__ void __launch_bounds__(64) hmm_emit_product(const double* __restrict__ x, int64_t n, int P, Par m, double2* __restrict__ B,
                                                       double* __restrict__ pm, double* __restrict__ acc) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int64_t a = n * p / P, b = n * (p + 1) / P;
    double m00 = 1, m01 = 0, m10 = 0, m11 = 1, ll = 0;
    for (int64_t t = a; t < b; ++t) {
        const double d0 = x[t] - m.mu0, d1 = x[t] - m.mu1;
        const double l0 = -0.5 * ((frisk_hmm::LOG2PI + m.lc0) + d0 * d0 * m.ic0), l1 = -0.5 * ((frisk_hmm::LOG2PI + m.lc1) + d1 * d1 * m.ic1);
        const double mx = fmax(l0, l1);
        const double b0 = exp(l0 - mx), b1 = exp(l1 - mx);
        B[t] = make_double2(b0, b1);
        ll += mx;
        if (t == 0) continue;                                   // (the first window's step is the start vector, not a transition)
        const double s00 = m.a00 * b0, s01 = m.a01 * b1, s10 = m.a10 * b0, s11 = m.a11 * b1;
        const double n00 = m00 * s00 + m01 * s10, n01 = m00 * s01 + m01 * s11;
        const double n10 = m10 * s00 + m11 * s10, n11 = m10 * s01 + m11 * s11;
        const double r = 1.0 / (n00 + n01 + n10 + n11);
        m00 = n00 * r; m01 = n01 * r; m10 = n10 * r; m11 = n11 * r;
    }
    pm[size_t(p) * 4] = m00; pm[size_t(p) * 4 + 1] = m01; pm[size_t(p) * 4 + 2] = m10; pm[size_t(p) * 4 + 3] = m11;
    acc[size_t(p) * ACC + 8] = ll;
}

// 2. the vectors at the cuts, serial over the pieces: lane 0 of wave 0 carries alpha forwards (edge[p] = normalised forward
//    vector in front of piece p; edge[0] = the UNnormalised first vector), lane 0 of wave 1 carries beta backwards
//    (edgeB[p + 1] = beta of piece p's last window; flat at the end)
__global__ void __launch_bounds__(128) hmm_cuts(const double* __restrict__ pm, int P, Par m, const double2* __restrict__ B,
                                                double* __restrict__ edge, double* __restrict__ edgeB) {
    if (threadIdx.x == 0) {
        const double2 b = B[0];
        double v0 = m.pi0 * b.x, v1 = m.pi1 * b.y;
        edge[0] = v0; edge[1] = v1;
        double s = v0 + v1;
        v0 /= s; v1 /= s;
        for (int p = 0; p + 1 < P; ++p) {
            const double* M = pm + size_t(p) * 4;
            const double w0 = v0 * M[0] + v1 * M[2], w1 = v0 * M[1] + v1 * M[3];
            s = w0 + w1;
            v0 = w0 / s; v1 = w1 / s;
            edge[size_t(p + 1) * 2] = v0; edge[size_t(p + 1) * 2 + 1] = v1;
        }
    } else if (threadIdx.x == 64) {
        double v0 = 0.5, v1 = 0.5;
        edgeB[size_t(P) * 2] = v0; edgeB[size_t(P) * 2 + 1] = v1;
        for (int p = P - 1; p >= 1; --p) {
            const double* M = pm + size_t(p) * 4;
            const double w0 = M[0] * v0 + M[1] * v1, w1 = M[2] * v0 + M[3] * v1;
            const double s = w0 + w1;
            v0 = w0 / s; v1 = w1 / s;
            edgeB[size_t(p) * 2] = v0; edgeB[size_t(p) * 2 + 1] = v1;
        }
    }
}

// 3. forward vectors of every window, and the scales' share of the log-likelihood
__global__ void __launch_bounds__(64) hmm_forward_walk(int64_t n, int P, Par m, const double2* __restrict__ B, const double* __restrict__ edge,
                                                       double2* __restrict__ A, double* __restrict__ acc) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int64_t a = n * p / P, b = n * (p + 1) / P;
    double v0, v1, ll = 0;
    int64_t t = a;
    if (p == 0) {
        const double s = edge[0] + edge[1];
        ll += log(s);
        v0 = edge[0] / s; v1 = edge[1] / s;
        A[0] = make_double2(v0, v1);
        t = 1;
    } else { v0 = edge[size_t(p) * 2]; v1 = edge[size_t(p) * 2 + 1]; }
    double prod = 1.0;                                          // the scales, four to a logarithm (each is >= the smallest transition
    int held = 0;                                               // probability: one of the two scaled emissions is exactly 1)
    for (; t < b; ++t) {
        const double2 e = B[t];
        const double w0 = (v0 * m.a00 + v1 * m.a10) * e.x, w1 = (v0 * m.a01 + v1 * m.a11) * e.y;
        const double s = w0 + w1, r = 1.0 / s;
        prod *= s;
        if (++held == 4 || prod < 1e-200) { ll += log(prod); prod = 1.0; held = 0; }
        v0 = w0 * r; v1 = w1 * r;
        A[t] = make_double2(v0, v1);
    }
    ll += log(prod);
    acc[size_t(p) * ACC + 9] = ll;
}

// 4. every piece backwards from the beta of its last window: posteriors (into A), transition posteriors, the M step's sums
__global__ void __launch_bounds__(64) hmm_backward_walk(const double* __restrict__ x, int64_t n, int P, Par m, const double2* __restrict__ B,
                                                        const double* __restrict__ edge, const double* __restrict__ edgeB,
                                                        double2* __restrict__ A, double* __restrict__ acc) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int64_t a = n * p / P, b = n * (p + 1) / P;
    double be0 = edgeB[size_t(p + 1) * 2], be1 = edgeB[size_t(p + 1) * 2 + 1];
    double g0s = 0, g1s = 0, gx0 = 0, gx1 = 0, x00 = 0, x01 = 0, x10 = 0, x11 = 0;
    for (int64_t t = b - 1; t >= a; --t) {
        const double2 al = A[t];
        double g0 = al.x * be0, g1 = al.y * be1;
        const double gr = 1.0 / (g0 + g1);
        g0 *= gr; g1 *= gr;
        A[t] = make_double2(g0, g1);
        const double xt = x[t];
        g0s += g0; g1s += g1; gx0 += g0 * xt; gx1 += g1 * xt;
        if (t == 0) break;
        const double2 e = B[t];
        const double b0 = e.x * be0, b1 = e.y * be1;
        // forward vector of window t-1: still in A inside the piece; the last window of the piece before is another thread's
        // (which turns it into a posterior) - its forward vector is the cut this piece started from
        double p0, p1;
        if (t > a) { const double2 pv = A[t - 1]; p0 = pv.x; p1 = pv.y; }
        else { p0 = edge[size_t(p) * 2]; p1 = edge[size_t(p) * 2 + 1]; }
        const double e00 = p0 * m.a00 * b0, e01 = p0 * m.a01 * b1, e10 = p1 * m.a10 * b0, e11 = p1 * m.a11 * b1;
        const double er = 1.0 / (e00 + e01 + e10 + e11);
        x00 += e00 * er; x01 += e01 * er; x10 += e10 * er; x11 += e11 * er;
        const double nb0 = m.a00 * b0 + m.a01 * b1, nb1 = m.a10 * b0 + m.a11 * b1;
        const double br = 1.0 / (nb0 + nb1);
        be0 = nb0 * br; be1 = nb1 * br;
    }
    double* q = acc + size_t(p) * ACC;
    q[0] = g0s; q[1] = g1s; q[2] = gx0; q[3] = gx1; q[4] = x00; q[5] = x01; q[6] = x10; q[7] = x11;
}

// 5. sum gamma (x - mu)^2 about the NEW means; cv[p * 2 + j]
__global__ void __launch_bounds__(64) hmm_covar_walk(const double* __restrict__ x, int64_t n, int P, double mu0, double mu1,
                                                     const double2* __restrict__ A, double* __restrict__ cv) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int64_t a = n * p / P, b = n * (p + 1) / P;
    double c0 = 0, c1 = 0;
    for (int64_t t = a; t < b; ++t) {
        const double d0 = x[t] - mu0, d1 = x[t] - mu1;
        const double2 g = A[t];
        c0 += g.x * (d0 * d0); c1 += g.y * (d1 * d1);
    }
    cv[size_t(p) * 2] = c0; cv[size_t(p) * 2 + 1] = c1;
}

// ---------------------------------------------------------------------------------------------------------------- host: fit
// the device arrays of one sequence: allocated once, used by every round
struct Work {
    frisk_common::DevMem mem;
    int P = 0, C = 0;
    double* dx = nullptr;
    double2 *B = nullptr, *A = nullptr;
    double *pm = nullptr, *edge = nullptr, *edgeB = nullptr, *acc = nullptr, *cv = nullptr, *part = nullptr, *out = nullptr;
    int load(const double* x, int64_t n) {
        P = pieces_of(n); C = parts_of(n);
        dx = mem.get<double>(size_t(n));
        B = mem.get<double2>(size_t(n));
        A = mem.get<double2>(size_t(n));
        pm = mem.get<double>(size_t(P) * 4);
        edge = mem.get<double>(size_t(P + 1) * 2);
        edgeB = mem.get<double>(size_t(P + 1) * 2);
        acc = mem.get<double>(size_t(P) * ACC);
        cv = mem.get<double>(size_t(P) * 2);
        part = mem.get<double>(size_t(PARTS) * 4);
        out = mem.get<double>(16);
        if (!dx || !B || !A || !pm || !edge || !edgeB || !acc || !cv || !part || !out) return -2;
        FRISK_HIP_CHECK(hipMemcpy(dx, x, size_t(n) * sizeof(double), hipMemcpyHostToDevice));
        return 0;
    }
};

// one E step of model m (what a round of fit runs, and all frisk_hmm_estep_gpu runs): the posteriors are left in w.A, the ACC
// sums in S (the log-likelihood is S[8] + S[9])
inline int e_step(const Work& w, int64_t n, const frisk_hmm::Model& m, double* S) {
    const int P = w.P;
    const unsigned gp = unsigned((P + 63) / 64);
    const Par par{m.means[0], m.means[1], std::log(m.covars[0]), std::log(m.covars[1]), 1.0 / m.covars[0], 1.0 / m.covars[1],
                  m.transmat[0], m.transmat[1], m.transmat[2], m.transmat[3], m.startprob[0], m.startprob[1]};
    hipLaunchKernelGGL(hmm_emit_product, dim3(gp), dim3(64), 0, 0, w.dx, n, P, par, w.B, w.pm, w.acc);
    hipLaunchKernelGGL(hmm_cuts, dim3(1), dim3(128), 0, 0, w.pm, P, par, w.B, w.edge, w.edgeB);
    hipLaunchKernelGGL(hmm_forward_walk, dim3(gp), dim3(64), 0, 0, n, P, par, w.B, w.edge, w.A, w.acc);
    hipLaunchKernelGGL(hmm_backward_walk, dim3(gp), dim3(64), 0, 0, w.dx, n, P, par, w.B, w.edge, w.edgeB, w.A, w.acc);
    hipLaunchKernelGGL(hmm_reduce_rows, dim3(1), dim3(RED_T), 0, 0, w.acc, P, ACC, w.out);
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(S, w.out, ACC * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// frisk_hmm_estep_gpu: post (n x 2, nullable), stats[9] = sum gamma (2), sum gamma x (2), sum xi (4), log-likelihood
inline int e_step_only(const double* x, int64_t n, const frisk_hmm::Model& m, double* post, double* stats) {
    Work w;
    if (w.load(x, n)) return -2;
    double S[ACC];
    if (e_step(w, n, m, S)) return -2;
    if (post) FRISK_HIP_CHECK(hipMemcpy(post, w.A, size_t(n) * 2 * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) stats[k] = S[k];
    stats[8] = S[8] + S[9];
    return 0;
}

inline int fit(const double* x, int64_t n, int n_iter, double tol, double min_covar, double covars_prior, frisk_hmm::Fit& F) {
    Work w;
    if (w.load(x, n)) return -2;
    const int P = w.P, C = w.C;
    double *dx = w.dx, *cv = w.cv, *part = w.part, *out = w.out;
    double2* A = w.A;
    double h[16];
    frisk_hmm::Model& m = F.m;
    // start (GaussianHMM2._init)
    hipLaunchKernelGGL(hmm_init_range, dim3(C), dim3(RED_T), 0, 0, dx, n, C, part);
    hipLaunchKernelGGL(hmm_init_range_final, dim3(1), dim3(RED_T), 0, 0, part, C, out);
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(h, out, 3 * sizeof(double), hipMemcpyDeviceToHost));
    double c[2] = {h[0], h[1]};
    const double mu = h[2] / double(n);
    for (int it = 0; it < 100; ++it) {
        hipLaunchKernelGGL(hmm_init_assign, dim3(C), dim3(RED_T), 0, 0, dx, n, C, c[0], c[1], part);
        hipLaunchKernelGGL(hmm_reduce_rows, dim3(1), dim3(RED_T), 0, 0, part, C, 4, out);
        FRISK_HIP_CHECK(hipGetLastError());
        FRISK_HIP_CHECK(hipMemcpy(h, out, 4 * sizeof(double), hipMemcpyDeviceToHost));
        const double nw[2] = {h[1] > 0 ? h[0] / h[1] : c[0], h[3] > 0 ? h[2] / h[3] : c[1]};
        // numpy.allclose(new, c); on convergence the centres of the PREVIOUS round are kept
        if (std::fabs(nw[0] - c[0]) <= 1e-8 + 1e-5 * std::fabs(c[0]) && std::fabs(nw[1] - c[1]) <= 1e-8 + 1e-5 * std::fabs(c[1])) break;
        c[0] = nw[0]; c[1] = nw[1];
    }
    m.means[0] = std::min(c[0], c[1]); m.means[1] = std::max(c[0], c[1]);
    hipLaunchKernelGGL(hmm_init_var, dim3(C), dim3(RED_T), 0, 0, dx, n, C, mu, part);
    hipLaunchKernelGGL(hmm_reduce_rows, dim3(1), dim3(RED_T), 0, 0, part, C, 1, out);
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(h, out, sizeof(double), hipMemcpyDeviceToHost));
    m.covars[0] = m.covars[1] = h[0] / double(n) + min_covar;
    m.startprob[0] = m.startprob[1] = 0.5;
    for (double& a : m.transmat) a = 0.5;
    F.loglik = -std::numeric_limits<double>::infinity();
    F.iters = 0;
    // Baum-Welch (GaussianHMM2.fit)
    const unsigned gp = unsigned((P + 63) / 64);
    double prev = -std::numeric_limits<double>::infinity();
    for (int it = 0; it < n_iter; ++it) {
        if (e_step(w, n, m, h)) return -2;
        double g[2];
        FRISK_HIP_CHECK(hipMemcpy(g, A, 2 * sizeof(double), hipMemcpyDeviceToHost));      // posterior of the first window
        const double* S = h;
        const double ll = S[8] + S[9];
        // M step (hmmlearn's defaults: flat Dirichlet priors, means_weight 0, covars_prior / weight 1e-2 / 1)
        m.startprob[0] = g[0] / (g[0] + g[1]); m.startprob[1] = g[1] / (g[0] + g[1]);
        if (n > 1) {
            const double r0 = S[4] + S[5], r1 = S[6] + S[7];
            m.transmat[0] = r0 > 0 ? S[4] / r0 : 0.5; m.transmat[1] = r0 > 0 ? S[5] / r0 : 0.5;
            m.transmat[2] = r1 > 0 ? S[6] / r1 : 0.5; m.transmat[3] = r1 > 0 ? S[7] / r1 : 0.5;
        } else { for (double& v : m.transmat) v = 0.5; }
        m.means[0] = S[2] / S[0]; m.means[1] = S[3] / S[1];
        const double w0 = S[0], w1 = S[1];
        hipLaunchKernelGGL(hmm_covar_walk, dim3(gp), dim3(64), 0, 0, dx, n, P, m.means[0], m.means[1], A, cv);
        hipLaunchKernelGGL(hmm_reduce_rows, dim3(1), dim3(RED_T), 0, 0, cv, P, 2, out);
        FRISK_HIP_CHECK(hipGetLastError());
        double cc[2];
        FRISK_HIP_CHECK(hipMemcpy(cc, out, 2 * sizeof(double), hipMemcpyDeviceToHost));
        m.covars[0] = std::max((covars_prior + cc[0]) / w0, 1e-300);
        m.covars[1] = std::max((covars_prior + cc[1]) / w1, 1e-300);
        F.loglik = ll;
        F.iters = it + 1;
        if (ll - prev < tol) break;                             // in double, on the host, once per round
        prev = ll;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- Viterbi
struct VPar {
    double mu0, mu1, cv0, cv1, lc0, lc1, t00, t01, t10, t11, ls0, ls1;      // logs taken on the host (as hmm_host.h takes them)
};

__device__ inline double hmm_loglik(double x, double mean, double covar, double logcov) {
    const double d = x - mean;
    return -0.5 * ((frisk_hmm::LOG2PI + logcov) + d * d / covar);
}

// 1. piece k = windows [pa[k], pb[k]) of one scaffold.  For each entry state e (the state of the window in front of the piece)
//    the best score of ending in state j, M[k][e][j], with the entry's own score taken as 0, and the backpointers of every
//    step: back[t] bit (2 e + j) = predecessor of state j at window t under entry e.  A scaffold's first piece starts from the
//    start vector instead (both rows equal).
__global__ void __launch_bounds__(64) hmm_vit_pieces(const double* __restrict__ x, const int64_t* __restrict__ pa, const int64_t* __restrict__ pb,
                                                     const uint8_t* __restrict__ pfirst, int64_t K, VPar m, uint8_t* __restrict__ back,
                                                     double* __restrict__ M) {
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int64_t a = pa[k], b = pb[k];
    const double e0 = hmm_loglik(x[a], m.mu0, m.cv0, m.lc0), e1 = hmm_loglik(x[a], m.mu1, m.cv1, m.lc1);
    double r00, r01, r10, r11;                                  // r[e][j]
    if (pfirst[k]) { r00 = r10 = m.ls0 + e0; r01 = r11 = m.ls1 + e1; }
    else { r00 = m.t00 + e0; r01 = m.t01 + e1; r10 = m.t10 + e0; r11 = m.t11 + e1; }
    back[a] = 0;
    for (int64_t t = a + 1; t < b; ++t) {
        const double l0 = hmm_loglik(x[t], m.mu0, m.cv0, m.lc0), l1 = hmm_loglik(x[t], m.mu1, m.cv1, m.lc1);
        unsigned bits = 0;
        {
            const double c00 = r00 + m.t00, c10 = r01 + m.t10, c01 = r00 + m.t01, c11 = r01 + m.t11;
            const unsigned k0 = c10 > c00 ? 1u : 0u, k1 = c11 > c01 ? 1u : 0u;
            bits |= k0 | (k1 << 1);
            r00 = (k0 ? c10 : c00) + l0; r01 = (k1 ? c11 : c01) + l1;
        }
        {
            const double c00 = r10 + m.t00, c10 = r11 + m.t10, c01 = r10 + m.t01, c11 = r11 + m.t11;
            const unsigned k0 = c10 > c00 ? 1u : 0u, k1 = c11 > c01 ? 1u : 0u;
            bits |= (k0 << 2) | (k1 << 3);
            r10 = (k0 ? c10 : c00) + l0; r11 = (k1 ? c11 : c01) + l1;
        }
        back[t] = uint8_t(bits);
    }
    double* q = M + size_t(k) * 4;
    q[0] = r00; q[1] = r01; q[2] = r10; q[3] = r11;
}

// 2. one thread per scaffold: the score vector across the cuts (relative to the better state), the entry state each end state
//    prefers, then - from the better final state backwards - every piece's end state and entry state
__global__ void __launch_bounds__(64) hmm_vit_cuts(const int64_t* __restrict__ seg_piece, int32_t n_seg, const double* __restrict__ M,
                                                   uint8_t* __restrict__ choice, uint8_t* __restrict__ endst, uint8_t* __restrict__ entry) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t k0 = seg_piece[s], k1 = seg_piece[s + 1];
    if (k1 <= k0) return;
    const double ninf = -std::numeric_limits<double>::infinity();
    double v0 = M[size_t(k0) * 4], v1 = M[size_t(k0) * 4 + 1];
    for (int64_t k = k0 + 1; k < k1; ++k) {
        const double mx = fmax(v0, v1);
        if (mx > ninf) { v0 -= mx; v1 -= mx; }
        const double* q = M + size_t(k) * 4;
        const double c00 = v0 + q[0], c10 = v1 + q[2], c01 = v0 + q[1], c11 = v1 + q[3];
        const unsigned h0 = c10 > c00 ? 1u : 0u, h1 = c11 > c01 ? 1u : 0u;
        choice[k] = uint8_t(h0 | (h1 << 1));
        v0 = h0 ? c10 : c00; v1 = h1 ? c11 : c01;
    }
    unsigned st = v1 > v0 ? 1u : 0u;
    for (int64_t k = k1 - 1; k >= k0; --k) {
        endst[k] = uint8_t(st);
        const unsigned e = k > k0 ? (choice[k] >> st) & 1u : 0u;
        entry[k] = uint8_t(e);
        st = e;
    }
}

// 3. backtrack every piece from its end state along the backpointers of its entry state
__global__ void __launch_bounds__(64) hmm_vit_backtrack(const int64_t* __restrict__ pa, const int64_t* __restrict__ pb, int64_t K,
                                                        const uint8_t* __restrict__ back, const uint8_t* __restrict__ endst,
                                                        const uint8_t* __restrict__ entry, int8_t* __restrict__ path) {
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int64_t a = pa[k], b = pb[k];
    unsigned cur = endst[k];
    const unsigned sh = 2u * entry[k];
    for (int64_t t = b - 1; t > a; --t) {
        path[t] = int8_t(cur);
        cur = (back[t] >> (sh + cur)) & 1u;
    }
    path[a] = int8_t(cur);
}

// sequences [off[s], off[s + 1]) of x into path (both indexed as off[] says); returns 0 or -2
inline int viterbi_segments(const double* x, const int64_t* off, int32_t n_seg, const frisk_hmm::Model& m, int8_t* path) {
    using frisk_common::DevMem;
    const int64_t base = off[0], n = off[n_seg] - off[0];
    if (n <= 0) return 0;
    std::vector<int64_t> pa, pb, seg_piece(size_t(n_seg) + 1);
    std::vector<uint8_t> pfirst;
    for (int32_t s = 0; s < n_seg; ++s) {
        seg_piece[size_t(s)] = int64_t(pa.size());
        for (int64_t a = off[s]; a < off[s + 1]; a += VIT_STEPS) {
            pa.push_back(a - base);
            pb.push_back(std::min<int64_t>(a + VIT_STEPS, off[s + 1]) - base);
            pfirst.push_back(a == off[s] ? 1 : 0);
        }
    }
    seg_piece[size_t(n_seg)] = int64_t(pa.size());
    const int64_t K = int64_t(pa.size());
    DevMem mem;
    double* dx = mem.get<double>(size_t(n));
    int64_t* dpa = mem.get<int64_t>(size_t(K));
    int64_t* dpb = mem.get<int64_t>(size_t(K));
    uint8_t* dfirst = mem.get<uint8_t>(size_t(K));
    int64_t* dseg = mem.get<int64_t>(size_t(n_seg) + 1);
    uint8_t* back = mem.get<uint8_t>(size_t(n));
    double* M = mem.get<double>(size_t(K) * 4);
    uint8_t* choice = mem.get<uint8_t>(size_t(K));
    uint8_t* endst = mem.get<uint8_t>(size_t(K));
    uint8_t* entry = mem.get<uint8_t>(size_t(K));
    int8_t* dpath = mem.get<int8_t>(size_t(n));
    if (!dx || !dpa || !dpb || !dfirst || !dseg || !back || !M || !choice || !endst || !entry || !dpath) return -2;
    FRISK_HIP_CHECK(hipMemcpy(dx, x + base, size_t(n) * sizeof(double), hipMemcpyHostToDevice));
    FRISK_HIP_CHECK(hipMemcpy(dpa, pa.data(), size_t(K) * sizeof(int64_t), hipMemcpyHostToDevice));
    FRISK_HIP_CHECK(hipMemcpy(dpb, pb.data(), size_t(K) * sizeof(int64_t), hipMemcpyHostToDevice));
    FRISK_HIP_CHECK(hipMemcpy(dfirst, pfirst.data(), size_t(K), hipMemcpyHostToDevice));
    FRISK_HIP_CHECK(hipMemcpy(dseg, seg_piece.data(), (size_t(n_seg) + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    const VPar par{m.means[0], m.means[1], m.covars[0], m.covars[1], std::log(m.covars[0]), std::log(m.covars[1]),
                   std::log(m.transmat[0]), std::log(m.transmat[1]), std::log(m.transmat[2]), std::log(m.transmat[3]),
                   std::log(m.startprob[0]), std::log(m.startprob[1])};
    const unsigned gk = unsigned((K + 63) / 64), gs = unsigned((int64_t(n_seg) + 63) / 64);
    hipLaunchKernelGGL(hmm_vit_pieces, dim3(gk), dim3(64), 0, 0, dx, dpa, dpb, dfirst, K, par, back, M);
    hipLaunchKernelGGL(hmm_vit_cuts, dim3(gs), dim3(64), 0, 0, dseg, n_seg, M, choice, endst, entry);
    hipLaunchKernelGGL(hmm_vit_backtrack, dim3(gk), dim3(64), 0, 0, dpa, dpb, K, back, endst, entry, dpath);
    FRISK_HIP_CHECK(hipGetLastError());
    FRISK_HIP_CHECK(hipMemcpy(path + base, dpath, size_t(n), hipMemcpyDeviceToHost));
    return 0;
}


}  // namespace frisk_hmm_gpu
