// frisk_analysis.hip - the entry points of include/frisk_hip.h that take no frisk_ctx: the host HMM, projection and clustering, the
// device HMM, and the t-SNE, MDS, incremental PCA, NMF and spectral-clustering handles.  Host arrays in and out, or a small handle of their own; nothing
// of the scan is included here.  gfx950 (MI355X) only.  Build: see __graft_entry__.build_hip().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "frisk_hip.h"
#include "hmm_host.h"
#include "analysis_common.h"
#include "proj_kernels.h"
#include "tsne_kernels.h"
#include "mds_kernels.h"
#include "ipca_kernels.h"
#include "nmf_kernels.h"
#include "spectral_kernels.h"
#include "skltsne_kernels.h"
#include "hmm_kernels.h"

namespace {

// switch to `device`, run f there, and map its non-zero result to FRISK_E_HIP
template <typename F>
int on_device(int device, F&& f) {
    frisk_common::OnDevice on(device);
    if (!on.ok) return FRISK_E_HIP;
    return f() ? FRISK_E_HIP : FRISK_OK;
}

// The handles (frisk_tsne, frisk_mds, frisk_ipca, frisk_nmf, frisk_spectral: one State `s` each, which frees its device memory when it is deleted on
// its device).  `make` fills the state's shape and allocates: 0, or the handle is dropped.
template <typename H, typename Make>
int create_handle(int device, H** out, Make&& make) {
    frisk_common::OnDevice on(device);
    if (!on.ok) return FRISK_E_HIP;
    H* h = new (std::nothrow) H;
    if (!h) return FRISK_E_HIP;
    h->s.device = device;
    if (make(h->s)) {
        delete h;
        return FRISK_E_HIP;
    }
    *out = h;
    return FRISK_OK;
}

template <typename H>
void destroy_handle(H* h) {
    if (!h) return;
    frisk_common::OnDevice on(h->s.device);
    delete h;
}

// ms[which] of a handle's last timed call (the *_last_ms entries), -1 for no handle or no such slot
template <typename H>
double last_ms(const H* h, int which) {
    return (h && which >= 0 && which < 3) ? h->s.ms[which] : -1.0;
}

// copy `bytes` between a host array the caller may have left out (null: nothing to do) and the device; true when the copy fails
bool copy_fails(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    return dst && src && hipMemcpy(dst, src, bytes, kind) != hipSuccess;
}

}  // namespace

extern "C" {

// ---- host-native 2-state Gaussian HMM (hmm_host.h): the model frisk_amd/hmm.py documents, for millions of windows ----------
namespace {
frisk_hmm::Model model_of(const double* means, const double* covars, const double* startprob, const double* transmat) {
    frisk_hmm::Model m;
    for (int i = 0; i < 2; ++i) { m.means[i] = means[i]; m.covars[i] = covars[i]; m.startprob[i] = startprob[i]; }
    for (int i = 0; i < 4; ++i) m.transmat[i] = transmat[i];
    return m;
}
int fit_out(const frisk_hmm::Fit& F, double* means, double* covars, double* startprob, double* transmat, double* loglik, int32_t* iters) {
    for (int i = 0; i < 2; ++i) { means[i] = F.m.means[i]; covars[i] = F.m.covars[i]; startprob[i] = F.m.startprob[i]; }
    for (int i = 0; i < 4; ++i) transmat[i] = F.m.transmat[i];
    if (loglik) *loglik = F.loglik;
    if (iters) *iters = F.iters;
    return FRISK_OK;
}
}  // namespace

int frisk_hmm_fit(const double* x, int64_t n, int32_t n_iter, double tol, double min_covar, double covars_prior, double* means,
                  double* covars, double* startprob, double* transmat, double* loglik, int32_t* iters) {
    if (!x || n < 1 || n_iter < 0 || !means || !covars || !startprob || !transmat) return FRISK_E_ARG;
    for (int64_t t = 0; t < n; ++t) if (!std::isfinite(x[t])) return FRISK_E_ARG;
    const frisk_hmm::Fit F = frisk_hmm::fit(x, n, n_iter, tol, min_covar, covars_prior);
    return fit_out(F, means, covars, startprob, transmat, loglik, iters);
}

int frisk_hmm_viterbi(const double* x, const int64_t* seg_off, int32_t n_seg, const double* means, const double* covars,
                      const double* startprob, const double* transmat, int8_t* states) {
    if (n_seg < 0 || !seg_off || !means || !covars || !startprob || !transmat) return FRISK_E_ARG;
    for (int32_t s = 0; s < n_seg; ++s) if (seg_off[s + 1] < seg_off[s]) return FRISK_E_ARG;
    if (n_seg == 0 || seg_off[n_seg] == seg_off[0]) return FRISK_OK;
    if (!x || !states) return FRISK_E_ARG;
    const frisk_hmm::Model m = model_of(means, covars, startprob, transmat);
    frisk_hmm::viterbi_segments(x, seg_off, n_seg, m, states);
    return FRISK_OK;
}

namespace {
// x and the model of one E step: finite, variances > 0, probabilities in [0, 1]
bool estep_args_ok(const double* x, int64_t n, const double* means, const double* covars, const double* startprob,
                   const double* transmat, const double* stats_out) {
    if (!x || n < 1 || !means || !covars || !startprob || !transmat || !stats_out) return false;
    for (int i = 0; i < 2; ++i) {
        if (!std::isfinite(means[i]) || !std::isfinite(covars[i]) || !(covars[i] > 0.0)) return false;
        if (!(startprob[i] >= 0.0 && startprob[i] <= 1.0)) return false;
    }
    for (int i = 0; i < 4; ++i) if (!(transmat[i] >= 0.0 && transmat[i] <= 1.0)) return false;
    for (int64_t t = 0; t < n; ++t) if (!std::isfinite(x[t])) return false;
    return true;
}
}  // namespace

int frisk_hmm_estep(const double* x, int64_t n, const double* means, const double* covars, const double* startprob,
                    const double* transmat, double* post_out, double* stats_out) {
    if (!estep_args_ok(x, n, means, covars, startprob, transmat, stats_out)) return FRISK_E_ARG;
    const frisk_hmm::Model m = model_of(means, covars, startprob, transmat);
    frisk_hmm::Work w(n);
    stats_out[8] = frisk_hmm::e_step(x, n, m, w, stats_out);
    if (post_out) std::copy(w.A.begin(), w.A.end(), post_out);
    return FRISK_OK;
}

// ---- projection and clustering (proj_kernels.h): context-free, host arrays in and out, device memory freed on every return
namespace {
bool all_finite(const double* x, int64_t count) {
    for (int64_t e = 0; e < count; ++e) if (!std::isfinite(x[e])) return false;
    return true;
}
}  // namespace

int frisk_proj_cov(int device, const double* X, int64_t n, int64_t f, double* mean_out, double* cov_out) {
    if (!X || !mean_out || !cov_out || n < 1 || f < 1 || !all_finite(X, n * f)) return FRISK_E_ARG;
    return on_device(device, [&] { return frisk_proj::cov(X, n, f, mean_out, cov_out); });
}

int frisk_proj_transform(int device, const double* X, const double* mean, const double* V, int64_t n, int64_t f, int32_t d,
                         double* Y_out) {
    if (!X || !mean || !V || !Y_out || n < 1 || f < 1 || d < 1 || d > f || !all_finite(X, n * f) || !all_finite(mean, f) ||
        !all_finite(V, f * d))
        return FRISK_E_ARG;
    return on_device(device, [&] { return frisk_proj::transform(X, mean, V, n, f, d, Y_out); });
}

int frisk_dbscan(int device, const double* Y, int64_t n, int32_t d, double eps, int32_t min_samples, int32_t* labels_out) {
    if (!Y || !labels_out || n < 1 || n > INT32_MAX || d < 1 || d > frisk_proj::MAX_DIMS || !(eps > 0.0) || !std::isfinite(eps) ||
        min_samples < 1 || !all_finite(Y, n * d))
        return FRISK_E_ARG;
    return on_device(device, [&] { return frisk_proj::dbscan(Y, n, d, eps, min_samples, labels_out); });
}

int frisk_kmeans(int device, const double* Y, int64_t n, int32_t d, int32_t k, const double* init_centers, int32_t max_iter,
                 double tol, int32_t* labels_out, double* centers_out, double* inertia_out, int32_t* n_iter_out) {
    if (!Y || !init_centers || !labels_out || !centers_out || n < 1 || n > INT32_MAX || d < 1 || d > frisk_proj::MAX_DIMS ||
        k < 1 || k > n || max_iter < 1 || !(tol >= 0.0) || !all_finite(Y, n * d) || !all_finite(init_centers, int64_t(k) * d))
        return FRISK_E_ARG;
    return on_device(device, [&] {
        return frisk_proj::kmeans(Y, n, d, k, init_centers, max_iter, tol, labels_out, centers_out, inertia_out, n_iter_out);
    });
}

// ---- the same HMM on the device (hmm_kernels.h): context-free, host arrays in and out, device memory freed on every return
int frisk_hmm_fit_gpu(int device, const double* x, int64_t n, int32_t n_iter, double tol, double min_covar, double covars_prior,
                      double* means, double* covars, double* startprob, double* transmat, double* loglik, int32_t* iters) {
    if (!x || n < 1 || n > (int64_t(1) << 40) || n_iter < 0 || !means || !covars || !startprob || !transmat || !all_finite(x, n))
        return FRISK_E_ARG;
    frisk_common::OnDevice on(device);
    if (!on.ok) return FRISK_E_HIP;
    frisk_hmm::Fit F;
    if (frisk_hmm_gpu::fit(x, n, n_iter, tol, min_covar, covars_prior, F)) return FRISK_E_HIP;
    return fit_out(F, means, covars, startprob, transmat, loglik, iters);
}

int frisk_hmm_estep_gpu(int device, const double* x, int64_t n, const double* means, const double* covars, const double* startprob,
                        const double* transmat, double* post_out, double* stats_out) {
    if (!estep_args_ok(x, n, means, covars, startprob, transmat, stats_out) || n > (int64_t(1) << 40)) return FRISK_E_ARG;
    const frisk_hmm::Model m = model_of(means, covars, startprob, transmat);
    return on_device(device, [&] { return frisk_hmm_gpu::e_step_only(x, n, m, post_out, stats_out); });
}

int frisk_hmm_viterbi_gpu(int device, const double* x, const int64_t* seg_off, int32_t n_seg, const double* means,
                          const double* covars, const double* startprob, const double* transmat, int8_t* states) {
    if (n_seg < 0 || !seg_off || !means || !covars || !startprob || !transmat) return FRISK_E_ARG;
    for (int32_t s = 0; s < n_seg; ++s) if (seg_off[s + 1] < seg_off[s]) return FRISK_E_ARG;
    if (n_seg == 0 || seg_off[n_seg] == seg_off[0]) return FRISK_OK;
    if (!x || !states || seg_off[n_seg] - seg_off[0] > (int64_t(1) << 40)) return FRISK_E_ARG;
    if (!all_finite(x + seg_off[0], seg_off[n_seg] - seg_off[0])) return FRISK_E_ARG;
    const frisk_hmm::Model m = model_of(means, covars, startprob, transmat);
    return on_device(device, [&] { return frisk_hmm_gpu::viterbi_segments(x, seg_off, n_seg, m, states); });
}

// ---- exact t-SNE (tsne_kernels.h): a handle whose state stays on its device between calls
struct frisk_tsne {
    frisk_tsne_impl::State s;
};

int frisk_tsne_create(int device, const double* X, int64_t n, int32_t f, double perplexity, int32_t dims, const double* Y0,
                      frisk_tsne** out) {
    if (!out) return FRISK_E_ARG;
    *out = nullptr;
    if (!X || !Y0 || n < 2 || n > frisk_tsne_impl::MAX_N || f < 1 || f > frisk_tsne_impl::MAX_F || dims < 1 ||
        dims > frisk_tsne_impl::MAX_D || !(perplexity > 0.0) || !std::isfinite(perplexity) || !all_finite(X, n * f) ||
        !all_finite(Y0, n * dims))
        return FRISK_E_ARG;
    return create_handle(device, out, [&](frisk_tsne_impl::State& s) {
        s.n = n; s.f = f; s.d = dims; s.perplexity = perplexity;
        return s.alloc(X, Y0);
    });
}

int frisk_tsne_affinities(frisk_tsne* h, double* beta_out, int32_t* tries_out, double* q_out) {
    if (!h) return FRISK_E_ARG;
    frisk_common::OnDevice on(h->s.device);
    if (!on.ok) return FRISK_E_HIP;
    const int64_t n = h->s.n;
    if (!h->s.have_p) {
        const int e = h->s.affinities();
        if (e) return e == -1 ? FRISK_E_ARG : FRISK_E_HIP;
    }
    if (copy_fails(beta_out, h->s.beta, size_t(n) * sizeof(double), hipMemcpyDeviceToHost) ||
        copy_fails(tries_out, h->s.tries, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost) ||
        copy_fails(q_out, h->s.P, size_t(n) * size_t(n) * sizeof(double), hipMemcpyDeviceToHost))
        return FRISK_E_HIP;
    return FRISK_OK;
}

int frisk_tsne_run(frisk_tsne* h, int32_t iter_begin, int32_t iter_end, double* cost_out) {
    if (!h || iter_begin < 0 || iter_end < iter_begin || iter_end > frisk_tsne_impl::MAX_ITER) return FRISK_E_ARG;
    frisk_common::OnDevice on(h->s.device);
    if (!on.ok) return FRISK_E_HIP;
    if (!h->s.have_p) {
        const int e = h->s.affinities();
        if (e) return e == -1 ? FRISK_E_ARG : FRISK_E_HIP;
    }
    return h->s.run(iter_begin, iter_end, cost_out) ? FRISK_E_HIP : FRISK_OK;
}

int frisk_tsne_get(frisk_tsne* h, double* Y, double* iY, double* gains) {
    if (!h) return FRISK_E_ARG;
    const size_t bytes = size_t(h->s.n) * size_t(h->s.d) * sizeof(double);
    return on_device(h->s.device, [&] {
        return copy_fails(Y, h->s.Y, bytes, hipMemcpyDeviceToHost) ||
               copy_fails(iY, h->s.iY, bytes, hipMemcpyDeviceToHost) ||
               copy_fails(gains, h->s.gains, bytes, hipMemcpyDeviceToHost);
    });
}

int frisk_tsne_set(frisk_tsne* h, const double* Y, const double* iY, const double* gains) {
    if (!h) return FRISK_E_ARG;
    const int64_t nd = h->s.n * h->s.d;
    if ((Y && !all_finite(Y, nd)) || (iY && !all_finite(iY, nd)) || (gains && !all_finite(gains, nd))) return FRISK_E_ARG;
    const size_t bytes = size_t(nd) * sizeof(double);
    return on_device(h->s.device, [&] {
        return copy_fails(h->s.Y, Y, bytes, hipMemcpyHostToDevice) ||
               copy_fails(h->s.iY, iY, bytes, hipMemcpyHostToDevice) ||
               copy_fails(h->s.gains, gains, bytes, hipMemcpyHostToDevice);
    });
}

void frisk_tsne_destroy(frisk_tsne* h) { destroy_handle(h); }

// ---- metric MDS (mds_kernels.h): a handle holding the dissimilarities on its device between runs
struct frisk_mds {
    frisk_mds_impl::State s;
};

int frisk_mds_create(int device, const double* X, int64_t n, int64_t f, int32_t dims, frisk_mds** out) {
    if (!out) return FRISK_E_ARG;
    *out = nullptr;
    if (!X || n < 2 || n > frisk_mds_impl::MAX_N || f < 1 || dims < 1 || dims > frisk_mds_impl::MAX_D || !all_finite(X, n * f))
        return FRISK_E_ARG;
    return create_handle(device, out, [&](frisk_mds_impl::State& s) { s.n = n; s.f = f; s.d = dims; return s.create(X); });
}

int frisk_mds_dissimilarities(frisk_mds* h, double* D_out) {
    if (!h || !D_out) return FRISK_E_ARG;
    const size_t bytes = size_t(h->s.n) * size_t(h->s.n) * sizeof(double);
    return on_device(h->s.device, [&] { return hipMemcpy(D_out, h->s.D, bytes, hipMemcpyDeviceToHost) != hipSuccess; });
}

int frisk_mds_run(frisk_mds* h, const double* Y0, int32_t max_iter, double eps, double* Y_out, double* stress_out,
                  int32_t* n_iter_out, double* stress_trace_out) {
    if (!h || !Y0 || !Y_out || max_iter < 1 || !(eps >= 0.0) || !std::isfinite(eps) || !all_finite(Y0, h->s.n * h->s.d))
        return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.run(Y0, max_iter, eps, Y_out, stress_out, n_iter_out, stress_trace_out); });
}

void frisk_mds_destroy(frisk_mds* h) { destroy_handle(h); }

// ---- incremental PCA (ipca_kernels.h): a handle holding the fit (rows seen, mean, variance, S, V) on its device between batches
struct frisk_ipca {
    frisk_ipca_impl::State s;
};

int frisk_ipca_create(int device, int64_t f, int32_t d, frisk_ipca** out) {
    if (!out) return FRISK_E_ARG;
    *out = nullptr;
    if (f < 1 || d < 1 || d > f) return FRISK_E_ARG;
    return create_handle(device, out, [&](frisk_ipca_impl::State& s) { s.f = f; s.d = d; return s.create(); });
}

int frisk_ipca_gram(frisk_ipca* h, const double* X, int64_t b, double* G_out) {
    if (!h || !X || !G_out || b < 1 || (h->s.seen == 0 && b < h->s.d) || !all_finite(X, b * h->s.f)) return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.gram(X, b, G_out); });
}

int frisk_ipca_commit(frisk_ipca* h, const double* S, const double* Vt) {
    if (!h || !S || !Vt || !all_finite(S, h->s.d) || !all_finite(Vt, int64_t(h->s.d) * h->s.f)) return FRISK_E_ARG;
    if (!h->s.pending_b) return FRISK_E_STATE;
    return on_device(h->s.device, [&] { return h->s.commit(S, Vt); });
}

int frisk_ipca_get(frisk_ipca* h, int64_t* n_seen, double* mean, double* var, double* S, double* Vt) {
    if (!h) return FRISK_E_ARG;
    if (n_seen) *n_seen = h->s.seen;
    if (!mean && !var && !S && !Vt) return FRISK_OK;
    if (!h->s.fitted) return FRISK_E_STATE;
    const size_t fb = size_t(h->s.f) * sizeof(double), db = size_t(h->s.d) * sizeof(double);
    return on_device(h->s.device, [&] {
        return copy_fails(mean, h->s.mean, fb, hipMemcpyDeviceToHost) ||
               copy_fails(var, h->s.var, fb, hipMemcpyDeviceToHost) ||
               copy_fails(S, h->s.S, db, hipMemcpyDeviceToHost) ||
               copy_fails(Vt, h->s.Vt, size_t(h->s.d) * fb, hipMemcpyDeviceToHost);
    });
}

int frisk_ipca_set(frisk_ipca* h, int64_t n_seen, const double* mean, const double* var, const double* S, const double* Vt) {
    if (!h || n_seen < 0) return FRISK_E_ARG;
    if (n_seen > 0 && (!mean || !var || !S || !Vt || !all_finite(mean, h->s.f) || !all_finite(var, h->s.f) ||
                       !all_finite(S, h->s.d) || !all_finite(Vt, int64_t(h->s.d) * h->s.f)))
        return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.set(n_seen, mean, var, S, Vt); });
}

int frisk_ipca_transform(frisk_ipca* h, const double* X, int64_t n, double* Y_out) {
    if (!h || !X || !Y_out || n < 1 || !all_finite(X, n * h->s.f)) return FRISK_E_ARG;
    if (!h->s.fitted) return FRISK_E_STATE;
    return on_device(h->s.device, [&] { return h->s.transform(X, n, Y_out); });
}

double frisk_ipca_last_ms(const frisk_ipca* h, int which) { return last_ms(h, which); }

void frisk_ipca_destroy(frisk_ipca* h) { destroy_handle(h); }

// ---- NMF (nmf_kernels.h): a handle holding X, W and H on its device between products and steps
struct frisk_nmf {
    frisk_nmf_impl::State s;
};

namespace {
bool all_finite_nonneg(const double* x, int64_t count) {
    for (int64_t e = 0; e < count; ++e) if (!std::isfinite(x[e]) || x[e] < 0.0) return false;
    return true;
}

// H[d][f] (host) <-> Ht[f][d] (device)
int nmf_put_H(frisk_nmf_impl::State& s, const double* H) {
    std::vector<double> t(size_t(s.f) * size_t(s.d));
    frisk_common::transpose(H, s.d, s.f, t.data());
    s.frozen = false;
    return hipMemcpy(s.Ht, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? 0 : -2;
}

int nmf_take_H(frisk_nmf_impl::State& s, double* H) {
    std::vector<double> t(size_t(s.f) * size_t(s.d));
    if (hipMemcpy(t.data(), s.Ht, t.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -2;
    frisk_common::transpose(t.data(), s.f, s.d, H);
    return 0;
}
}  // namespace

int frisk_nmf_create(int device, const double* X, int64_t n, int64_t f, int32_t d, frisk_nmf** out) {
    if (!out) return FRISK_E_ARG;
    *out = nullptr;
    if (!X || n < 1 || f < 1 || d < 1 || d > frisk_nmf_impl::NMF_MAX_D || !all_finite_nonneg(X, n * f)) return FRISK_E_ARG;
    return create_handle(device, out, [&](frisk_nmf_impl::State& s) { s.n = n; s.f = f; s.d = d; return s.create(X); });
}

int frisk_nmf_xq(frisk_nmf* h, const double* Q, int32_t p, double* Y_out) {
    if (!h || !Q || !Y_out || p < 1 || p > frisk_nmf_impl::NMF_MAX_P || !all_finite(Q, h->s.f * p)) return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.xq(Q, p, Y_out); });
}

int frisk_nmf_xtq(frisk_nmf* h, const double* Q, int32_t p, double* Z_out) {
    if (!h || !Q || !Z_out || p < 1 || p > frisk_nmf_impl::NMF_MAX_P || !all_finite(Q, h->s.n * p)) return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.xtq(Q, p, Z_out); });
}

int frisk_nmf_set(frisk_nmf* h, const double* W, const double* H) {
    if (!h) return FRISK_E_ARG;
    if ((W && !all_finite(W, h->s.n * h->s.d)) || (H && !all_finite(H, int64_t(h->s.d) * h->s.f))) return FRISK_E_ARG;
    return on_device(h->s.device, [&] {
        return copy_fails(h->s.W, W, size_t(h->s.n) * size_t(h->s.d) * sizeof(double), hipMemcpyHostToDevice) ||
               (H && nmf_put_H(h->s, H));
    });
}

int frisk_nmf_get(frisk_nmf* h, double* W, double* H) {
    if (!h) return FRISK_E_ARG;
    return on_device(h->s.device, [&] {
        return copy_fails(W, h->s.W, size_t(h->s.n) * size_t(h->s.d) * sizeof(double), hipMemcpyDeviceToHost) ||
               (H && nmf_take_H(h->s, H));
    });
}

int frisk_nmf_step(frisk_nmf* h, double* W_inout, double* H_inout, int32_t update_H, double* violation) {
    if (!h || !violation) return FRISK_E_ARG;
    if (int e = frisk_nmf_set(h, W_inout, H_inout)) return e;
    frisk_common::OnDevice on(h->s.device);
    if (!on.ok) return FRISK_E_HIP;
    if (h->s.step(update_H ? 1 : 0, violation)) return FRISK_E_HIP;
    return frisk_nmf_get(h, W_inout, H_inout);
}

int frisk_nmf_transform_prepare(frisk_nmf* h) {
    if (!h) return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.prepare(); });
}

double frisk_nmf_last_ms(const frisk_nmf* h, int which) { return last_ms(h, which); }

void frisk_nmf_destroy(frisk_nmf* h) { destroy_handle(h); }

// ---- spectral clustering (spectral_kernels.h): a handle holding M = D^-1/2 A0 D^-1/2 and dd on its device between products
struct frisk_spectral {
    frisk_spectral_impl::State s;
};

int frisk_spectral_create(int device, const double* Y, int64_t n, int32_t d, double gamma, frisk_spectral** out) {
    if (!out) return FRISK_E_ARG;
    *out = nullptr;
    if (!Y || n < 2 || n > frisk_spectral_impl::MAX_N || d < 1 || d > frisk_proj::MAX_DIMS || !(gamma > 0.0) || !std::isfinite(gamma) ||
        !all_finite(Y, n * d))
        return FRISK_E_ARG;
    return create_handle(device, out, [&](frisk_spectral_impl::State& s) { s.n = n; s.d = d; s.gamma = gamma; return s.create(Y); });
}

int frisk_spectral_affinity(frisk_spectral* h, double* A0_out) {
    if (!h || !A0_out) return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.affinity(A0_out); });
}

int frisk_spectral_degrees(frisk_spectral* h, double* dd_out, int64_t* n_isolated) {
    if (!h || !dd_out || !n_isolated) return FRISK_E_ARG;
    *n_isolated = h->s.n_isolated;
    return on_device(h->s.device, [&] {
        return hipMemcpy(dd_out, h->s.dd, size_t(h->s.n) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess;
    });
}

int frisk_spectral_matrix(frisk_spectral* h, double* M_out) {
    if (!h || !M_out) return FRISK_E_ARG;
    const size_t bytes = size_t(h->s.n) * size_t(h->s.n) * sizeof(double);
    return on_device(h->s.device, [&] { return hipMemcpy(M_out, h->s.A, bytes, hipMemcpyDeviceToHost) != hipSuccess; });
}

int frisk_spectral_mq(frisk_spectral* h, const double* Q, int32_t p, double* Z_out) {
    if (!h || !Q || !Z_out || p < 1 || p > frisk_spectral_impl::SPECTRAL_MAX_P || !all_finite(Q, h->s.n * p)) return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.mq(Q, p, Z_out); });
}

double frisk_spectral_last_ms(const frisk_spectral* h, int which) { return last_ms(h, which); }

void frisk_spectral_destroy(frisk_spectral* h) { destroy_handle(h); }

// ---- sklearn's t-SNE (skltsne_kernels.h): a handle whose affinities and float32 state stay on its device between calls
struct frisk_skltsne {
    frisk_skltsne_impl::State s;
};

namespace {
bool all_finite32(const float* x, int64_t count) {
    for (int64_t e = 0; e < count; ++e) if (!std::isfinite(x[e])) return false;
    return true;
}
}  // namespace

int frisk_skltsne_create(int device, const double* X, int64_t n, int64_t f, double perplexity, int32_t dims, int32_t method,
                         frisk_skltsne** out) {
    namespace I = frisk_skltsne_impl;
    if (!out) return FRISK_E_ARG;
    *out = nullptr;
    if (!X || n < 2 || n > I::MAX_N || f < 1 || (method != I::METHOD_EXACT && method != I::METHOD_BARNES_HUT) || dims < 1 ||
        dims > (method == I::METHOD_EXACT ? I::MAX_D : I::MAX_D_BH) || !(perplexity > 0.0) || !(perplexity < double(n)) ||
        !all_finite(X, n * f))
        return FRISK_E_ARG;
    return create_handle(device, out, [&](I::State& s) {
        s.n = n; s.f = f; s.d = dims; s.method = method; s.perplexity = perplexity;
        return s.create(X);
    });
}

int frisk_skltsne_affinities(frisk_skltsne* h, double* beta_out, int32_t* steps_out) {
    if (!h) return FRISK_E_ARG;
    frisk_common::OnDevice on(h->s.device);
    if (!on.ok) return FRISK_E_HIP;
    if (h->s.affinities()) return FRISK_E_HIP;
    const size_t n = size_t(h->s.n);
    if (copy_fails(beta_out, h->s.beta, n * sizeof(double), hipMemcpyDeviceToHost) ||
        copy_fails(steps_out, h->s.steps, n * sizeof(int32_t), hipMemcpyDeviceToHost))
        return FRISK_E_HIP;
    return FRISK_OK;
}

int frisk_skltsne_p_dense(frisk_skltsne* h, double* P_out) {
    if (!h || !P_out) return FRISK_E_ARG;
    if (h->s.method != frisk_skltsne_impl::METHOD_EXACT || !h->s.have_aff) return FRISK_E_STATE;
    const size_t bytes = size_t(h->s.n) * size_t(h->s.n) * sizeof(double);
    return on_device(h->s.device, [&] { return hipMemcpy(P_out, h->s.P, bytes, hipMemcpyDeviceToHost) != hipSuccess; });
}

int frisk_skltsne_neighbours(frisk_skltsne* h, int32_t* indices_out, double* cond_out) {
    if (!h) return FRISK_E_ARG;
    if (h->s.method != frisk_skltsne_impl::METHOD_BARNES_HUT || !h->s.have_aff) return FRISK_E_STATE;
    const size_t nk = size_t(h->s.n) * size_t(h->s.k);
    return on_device(h->s.device, [&] {
        return copy_fails(indices_out, h->s.idx, nk * sizeof(int32_t), hipMemcpyDeviceToHost) ||
               copy_fails(cond_out, h->s.cond, nk * sizeof(double), hipMemcpyDeviceToHost);
    });
}

int frisk_skltsne_set_p(frisk_skltsne* h, const int64_t* indptr, const int32_t* indices, const float* values, int64_t nnz) {
    if (!h || !indptr || nnz < 0 || (nnz && (!indices || !values))) return FRISK_E_ARG;
    if (h->s.method != frisk_skltsne_impl::METHOD_BARNES_HUT) return FRISK_E_STATE;
    const int64_t n = h->s.n;
    if (indptr[0] != 0 || indptr[n] != nnz) return FRISK_E_ARG;
    for (int64_t i = 0; i < n; ++i) if (indptr[i + 1] < indptr[i]) return FRISK_E_ARG;
    for (int64_t e = 0; e < nnz; ++e) if (indices[e] < 0 || indices[e] >= n) return FRISK_E_ARG;
    if (!all_finite32(values, nnz)) return FRISK_E_ARG;
    return on_device(h->s.device, [&] { return h->s.set_p(indptr, indices, values, nnz); });
}

int frisk_skltsne_get(frisk_skltsne* h, float* Y, float* update, float* gains) {
    if (!h) return FRISK_E_ARG;
    const size_t bytes = size_t(h->s.n) * size_t(h->s.d) * sizeof(float);
    return on_device(h->s.device, [&] {
        return copy_fails(Y, h->s.Y, bytes, hipMemcpyDeviceToHost) ||
               copy_fails(update, h->s.U, bytes, hipMemcpyDeviceToHost) ||
               copy_fails(gains, h->s.G, bytes, hipMemcpyDeviceToHost);
    });
}

int frisk_skltsne_set(frisk_skltsne* h, const float* Y, const float* update, const float* gains) {
    if (!h) return FRISK_E_ARG;
    const int64_t nd = h->s.n * h->s.d;
    if ((Y && !all_finite32(Y, nd)) || (update && !all_finite32(update, nd)) || (gains && !all_finite32(gains, nd))) return FRISK_E_ARG;
    const size_t bytes = size_t(nd) * sizeof(float);
    return on_device(h->s.device, [&] {
        return copy_fails(h->s.Y, Y, bytes, hipMemcpyHostToDevice) ||
               copy_fails(h->s.U, update, bytes, hipMemcpyHostToDevice) ||
               copy_fails(h->s.G, gains, bytes, hipMemcpyHostToDevice) || (Y && h->s.refresh());
    });
}

int frisk_skltsne_run(frisk_skltsne* h, int32_t iter_begin, int32_t iter_end, double momentum, double exaggeration, double* error,
                      double* grad_norm) {
    if (!h || !error || !grad_norm || iter_begin < 0 || iter_end <= iter_begin || iter_end > frisk_skltsne_impl::MAX_ITER ||
        !std::isfinite(momentum) || !std::isfinite(exaggeration) || !(exaggeration > 0.0))
        return FRISK_E_ARG;
    frisk_common::OnDevice on(h->s.device);
    if (!on.ok) return FRISK_E_HIP;
    if (h->s.method == frisk_skltsne_impl::METHOD_BARNES_HUT) {
        if (!h->s.have_p) return FRISK_E_STATE;         // the symmetrised CSR comes from the caller (frisk_skltsne_set_p)
    } else if (h->s.affinities()) {
        return FRISK_E_HIP;
    }
    return h->s.run(iter_begin, iter_end, momentum, exaggeration, error, grad_norm) ? FRISK_E_HIP : FRISK_OK;
}

double frisk_skltsne_last_ms(const frisk_skltsne* h, int which) { return last_ms(h, which); }

void frisk_skltsne_destroy(frisk_skltsne* h) { destroy_handle(h); }

}  // extern "C"
